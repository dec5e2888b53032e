// plan_call_baseband (csrc/fmd_call_plan.hpp) against plan_call, under AddressSanitizer + UndefinedBehaviorSanitizer:
// for every geometry of the table a stream of calls whose sizes sweep 1 .. 65536, each call at the positions the one
// before left; the plan of the call's samples N and the plan of its baseband length M, at the same resampler position
// and feed count, have to agree in the code, the refusal sentence, M, R, A, every half-band stage's input count and
// regime, rs_pos (bit for bit) and the feed's counts -- and the baseband plan has no decimator phase (if_pos 0: the
// caller keeps its own).  One line "geometry <g> calls <n> accepted <a> refused <r> mismatches <m>" per geometry, a
// line "mismatch ..." for the first few; then the baseband plan's own refusals, one line each.  Built, run and read
// by tests/test_call_plan_baseband_cpu.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pvr.rtl.radiofm_amd/csrc/fmd_call_plan.hpp"
#include "../../pvr.rtl.radiofm_amd/csrc/fmd_design.hpp"

static fmd::Design design(double fs, unsigned D, double pcm)
{
  fmd::Params p;
  p.sample_rate_if = fs;
  p.tuning_offset = -0.15 * fs;
  p.sample_rate_pcm = pcm;
  p.downsample = D;
  return fmd::make_design(p);
}

static bool same(const fmd::CallPlan& a, const fmd::CallPlan& b, int ra, int rb, bool sentence)
{
  bool ok = ra == rb && a.M == b.M && a.R == b.R && a.A == b.A && a.feed_p0 == b.feed_p0 && a.feed_n == b.feed_n &&
            std::memcmp(&a.rs_pos, &b.rs_pos, sizeof(float)) == 0;
  for (unsigned s = 0; s < fmd::kMaxHbStages; s++)
    ok = ok && a.hb_in[s] == b.hb_in[s] && a.hb_mode[s] == b.hb_mode[s];
  if (sentence) // (the same words: the sentences are string literals of the one shared body)
    ok = ok && ((!a.why && !b.why) || (a.why && b.why && std::strcmp(a.why, b.why) == 0));
  return ok;
}

int main()
{
  // the design geometries of tests/cpp/call_plan_check.cpp, and the two whose decimators refuse by parity and length
  // (CIC stages at 6.4 MS/s, the 11-tap class at 600 kS/s)
  const struct
  {
    double fs;
    unsigned D;
    double pcm;
  } geo[] = {{2.4e6, 11, 48000.0}, {2.4e6, 11, 44100.0}, {1.0e6, 4, 48000.0}, {6.4e6, 1, 48000.0}, {2.4e6, 4, 48000.0}};
  std::vector<unsigned> sizes;
  for (unsigned n = 1; n <= 3000; n++)
    sizes.push_back(n);
  for (unsigned n = 3001; n <= 65536; n += 97)
    sizes.push_back(n);
  sizes.push_back(65535);
  sizes.push_back(65536);
  for (unsigned g = 0; g < sizeof(geo) / sizeof(geo[0]); g++)
  {
    const fmd::Design d = design(geo[g].fs, geo[g].D, geo[g].pcm);
    unsigned if_pos = 0, accepted = 0, refused = 0, bad = 0;
    float rs_pos = 0.0f;
    uint64_t feed_g = 0;
    for (unsigned n : sizes)
    {
      fmd::CallPlan pl, pb;
      const int rc = fmd::plan_call(d, if_pos, rs_pos, feed_g, 2, n, pl);
      const int rb = fmd::plan_call_baseband(d, rs_pos, feed_g, 2, pl.M, pb);
      // (M == 0 has its own words in each plan; the length test of an IQ call looks at the phase-0 length, which is
      // M or M + 1: at that one boundary the codes may differ, nowhere in this table)
      const bool sentence = pl.M != 0;
      if (!same(pl, pb, rc, rb, sentence) || pb.if_pos != 0)
      {
        if (bad++ < 5)
          std::printf("mismatch geometry %u samples %u: code %d / %d, M %u / %u, R %u / %u, A %u / %u, why %s / %s\n", g,
                      n, rc, rb, pl.M, pb.M, pl.R, pb.R, pl.A, pb.A, pl.why ? pl.why : "-", pb.why ? pb.why : "-");
      }
      if (rc != FMD_OK)
      {
        refused++;
        continue; // (a refused call leaves the positions where they were)
      }
      accepted++;
      if_pos = pl.if_pos;
      rs_pos = pl.rs_pos;
      feed_g += pl.A;
    }
    std::printf("geometry %u calls %zu accepted %u refused %u mismatches %u\n", g, sizes.size(), accepted, refused, bad);
  }
  // the baseband plan's refusals, one input each: no samples, nothing at the RDS rate, M + 51 > 32768 (and the largest
  // M below it), an odd block in front of a CIC stage, 19 samples in front of the 11-tap stage, no audio frame
  const struct
  {
    double fs;
    unsigned D;
    float rs_pos;
    unsigned M;
  } refusals[] = {{2.4e6, 11, 0.0f, 0},     {2.4e6, 11, 0.0f, 1},  {2.4e6, 1, 0.0f, 32718}, {2.4e6, 1, 0.0f, 32717},
                  {6.4e6, 1, 0.0f, 1001}, {2.4e6, 4, 0.0f, 19}, {2.4e6, 11, 100.0f, 50}};
  for (const auto& r : refusals)
  {
    fmd::CallPlan pl;
    const int rc = fmd::plan_call_baseband(design(r.fs, r.D, 48000.0), r.rs_pos, 0, 0, r.M, pl);
    std::printf("refusal %u %d %s\n", r.M, rc, pl.why ? pl.why : "-");
  }
  return 0;
}
