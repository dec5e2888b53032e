// The position plan of a call (csrc/fmd_call_plan.hpp) on its own, under AddressSanitizer + UndefinedBehaviorSanitizer:
// for every geometry of the table a sequence of call sizes, each call at the positions the one before left, one line
// "plan <geometry> <samples> <code> <M> <R> <A>" per call; then one line "refusal <samples> <code> <sentence>" for
// one input of each of the plan's size refusals.  Built, run and compared with the oracle's block lengths by
// tests/test_call_plan_cpu.py.
#include <cstdio>
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

int main()
{
  const struct
  {
    double fs;
    unsigned D;
    double pcm;
    unsigned min_samples;
  } geo[] = {{2.4e6, 11, 48000.0, 0}, {2.4e6, 11, 44100.0, 0}, {1.0e6, 4, 48000.0, 176}};
  const unsigned sizes[] = {8192, 20001, 8193, 65536, 12001, 88, 89, 30001, 8192, 9001, 176, 65535};
  for (unsigned g = 0; g < 3; g++)
  {
    const fmd::Design d = design(geo[g].fs, geo[g].D, geo[g].pcm);
    unsigned if_pos = 0;
    float rs_pos = 0.0f;
    uint64_t feed_g = 0;
    for (unsigned n : sizes)
    {
      if (n < geo[g].min_samples)
        continue;
      fmd::CallPlan pl;
      const int rc = fmd::plan_call(d, if_pos, rs_pos, feed_g, 2, n, pl);
      std::printf("plan %u %u %d %u %u %u\n", g, n, rc, pl.M, pl.R, pl.A);
      if (rc != FMD_OK)
        continue; // (a refused call leaves the positions where they were)
      if_pos = pl.if_pos;
      rs_pos = pl.rs_pos;
      feed_g += pl.A;
    }
  }
  // every size refusal once: at 2.4 MS/s, D = 11 no samples and one sample; the others where they can be met -- a
  // block of 65536 undecimated, an odd block in front of a CIC stage (6.4 MS/s), 19 baseband samples in front of the
  // 11-tap stage (600 kS/s), and a resampler position behind the block's end
  const struct
  {
    double fs;
    unsigned D;
    float rs_pos;
    unsigned samples;
  } refusals[] = {{2.4e6, 11, 0.0f, 0},  {2.4e6, 11, 0.0f, 1},   {2.4e6, 1, 0.0f, 65536},
                  {6.4e6, 1, 0.0f, 1001}, {2.4e6, 4, 0.0f, 76},   {2.4e6, 11, 100.0f, 550}};
  for (const auto& r : refusals)
  {
    fmd::CallPlan pl;
    const int rc = fmd::plan_call(design(r.fs, r.D, 48000.0), 0, r.rs_pos, 0, 0, r.samples, pl);
    std::printf("refusal %u %d %s\n", r.samples, rc, pl.why ? pl.why : "-");
  }
  return 0;
}
