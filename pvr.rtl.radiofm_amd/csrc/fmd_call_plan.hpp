/*
 * fmd_call_plan.hpp -- the position plan of one call: what a block of `samples` becomes at every rate of the chain,
 * from the design and the batch-uniform positions alone (the reference's bookkeeping: DownConvert.cpp:112-132,
 * 203-232).  A pure host function: the call path takes its lengths from it, and so does every check that has to know
 * them before anything is submitted.
 */
#pragma once

#include <cstdint>

#include "../../include/fmd.h"
#include "fmd_design.hpp"

namespace fmd
{

// Per stage of the half-band chain: how many inputs it sees and which of the reference's regimes
// that is (see k_hb_pass / k_roll_hb_mixed): HB_PASS below L inputs, HB_MIXED below 2 (L - 1).
enum HbMode { HB_NORMAL, HB_MIXED, HB_PASS };

constexpr unsigned kMaxHbStages = 9; // make_design refuses a longer chain (DownConvert.h:63, 168)

struct CallPlan
{
  unsigned M = 0;                // baseband length (DownConvert.cpp:112,123)
  unsigned R = 0;                // samples at the RDS rate
  unsigned A = 0;                // audio frames
  unsigned hb_in[kMaxHbStages] = {};
  HbMode hb_mode[kMaxHbStages] = {};
  unsigned if_pos = 0;           // the positions behind the call (if_pos: of a call that is not refused)
  float rs_pos = 0;
  unsigned feed_p0 = 0, feed_n = 0; // the call's first frame with a feed sample, its feed samples (0 with the feed off)
  const char* why = nullptr;     // the sentence of a refusal
};

/* The feed samples of a call of A frames behind g0 frames: the outputs n with g0 <= n D < g0 + A; *p0 = the call's
 * first frame that has one. */
inline unsigned feed_samples_of(uint64_t g0, unsigned A, unsigned D, unsigned* p0 = nullptr)
{
  const uint64_t first = (g0 + D - 1) / D;
  if (p0)
    *p0 = unsigned(first * D - g0);
  return unsigned((g0 + A + D - 1) / D - first);
}

/* What both kinds of call share: the plan of a call of baseband length M at resampler position rs_pos -- everything
 * behind the IF stage depends on the input through M alone.  m_long: the length the reference's half-band buffers are
 * tested against; m0_why: the refusal of M == 0.  if_pos is the caller's to set behind FMD_OK. */
inline int plan_baseband_body(const Design& d, float rs_pos, uint64_t feed_g, unsigned feed_div, unsigned M,
                              unsigned m_long, const char* m0_why, CallPlan& pl)
{
  auto refuse = [&](const char* why) {
    pl.why = why;
    return int(FMD_ERR_SIZE);
  };
  pl = CallPlan();
  pl.M = M;
  // fractional resampler walk (DownConvert.cpp:203-232), float arithmetic as written there
  const float p = rs_pos;
  const float pstep = d.rs_step;
  unsigned A = 0;
  float pf = p;
  unsigned pi = unsigned(int(pf));
  while (pi < M)
  {
    A++;
    pf = p + float(A) * pstep;
    pi = unsigned(int(pf));
  }
  pl.A = A;
  pl.rs_pos = pf - float(M); // DownConvert.cpp:230-232
  if (pl.rs_pos < 0)
    pl.rs_pos = 0;
  // the feed of the call: its first output and its sample count, from the frames of the feed calls so far
  if (feed_div)
    pl.feed_n = feed_samples_of(feed_g, A, feed_div, &pl.feed_p0);

  if (M == 0)
    return refuse(m0_why);
  // the reference's half-band delay lines hold 32768 samples (DownConvert.cpp:267,500); longer
  // baseband blocks overrun its heap, so they are outside the contract here too
  if (m_long + 51 > 32768)
    return refuse("baseband block longer than the reference's half-band buffers (32768)");
  unsigned R = M;
  for (size_t s = 0; s < d.hb.size() && s < kMaxHbStages; s++)
  {
    pl.hb_in[s] = R;
    const unsigned L = unsigned(d.hb[s].len);
    if (d.hb[s].cic)
    { // CCicN3DecimateBy2: "InLength must be an even number" (DownConvert.cpp:701) -- with an odd one the class
      // reads one sample past its block (whatever the buffer holds): outside the contract here
      if (R % 2u || R < 2u)
        return refuse("at this baseband rate the RDS decimator starts with CIC stages: the baseband length "
                      "of a call must be a multiple of 2 per CIC stage (the reference reads past an odd block)");
      R = R / 2; // :726
    }
    else if (L == 11)
    { // the unrolled class reads InLength - 10 .. and its first nine outputs unconditionally (:596-661)
      if (R < 20)
        return refuse("block too short for the 11-tap half-band stage");
      R = R / 2; // :688
    }
    else if (R < L)
    {
      pl.hb_mode[s] = HB_PASS;
      R = R / 2; // :519-520
    }
    else
    { // one output per even input index (:526-543)
      pl.hb_mode[s] = R >= 2u * (L - 1u) ? HB_NORMAL : HB_MIXED;
      R = (R + 1) / 2;
    }
  }
  pl.R = R;
  if (R == 0)
    return refuse("block too short: no sample reaches the RDS rate");
  if (A == 0)
    return refuse("block too short: no audio frame falls into it");
  return FMD_OK;
}

/* The plan of a call of `samples` at decimator phase if_pos and resampler position rs_pos; feed_div != 0: behind
 * feed_g frames of feed calls.  FMD_OK, or FMD_ERR_SIZE with the sentence in pl.why.  M, A and the feed's counts are
 * the call's whether or not it is refused (0 where no sample gets that far): a stride check in front of the refusal
 * reads them. */
inline int plan_call(const Design& d, unsigned if_pos, float rs_pos, uint64_t feed_g, unsigned feed_div,
                     unsigned samples, CallPlan& pl)
{
  const unsigned N = samples, D = d.D;
  const unsigned M = if_pos < N ? (N - if_pos + D - 1) / D : 0; // DownConvert.cpp:112,123
  const int rc = plan_baseband_body(d, rs_pos, feed_g, feed_div, M, (N + D - 1) / D,
                                    "block shorter than the decimator phase", pl);
  if (rc == FMD_OK)
    pl.if_pos = if_pos + M * D - N; // DownConvert.cpp:132
  return rc;
}

/* The plan of a call that brings its baseband itself (FMD_IN_CIQ_*: M complex samples per channel, the IF stage does
 * not run): M, R, A, the half-band regimes, rs_pos and the feed's counts are those of an IQ call that produces M
 * baseband samples, with the same refusal sentences; the decimator phase is not the call's (pl.if_pos stays 0: the
 * caller keeps its own). */
inline int plan_call_baseband(const Design& d, float rs_pos, uint64_t feed_g, unsigned feed_div, unsigned M,
                              CallPlan& pl)
{
  return plan_baseband_body(d, rs_pos, feed_g, feed_div, M, M, "a call of no baseband samples", pl);
}

} // namespace fmd
