/*
 * fmd_loud.hpp -- the host side of the loudness meter that needs no device (include/fmd.h, "ITU-R BS.1770 loudness
 * blocks"): the design of the two K-weighting biquads at the PCM rate, and the arithmetic over block records --
 * window loudness and the gated integrated loudness of BS.1770-4.  All of it in double.
 */
#pragma once

#include <cmath>
#include <vector>

#include "../../include/fmd.h"

namespace fmd
{

/* out[0..4] = b0 b1 b2 a1 a2 of the high shelf, out[5..9] of the high-pass: designed in double from the analogue
 * prototype's constants (at 48 kHz the table of BS.1770-4 to 1e-15), rounded once to float. */
inline void loud_design(double fs, float out[10])
{
  const double pi = 3.14159265358979323846;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    out[0] = float((Vh + Vb * K / Q + K * K) / a0);
    out[1] = float(2.0 * (K * K - Vh) / a0);
    out[2] = float((Vh - Vb * K / Q + K * K) / a0);
    out[3] = float(2.0 * (K * K - 1.0) / a0);
    out[4] = float((1.0 - K / Q + K * K) / a0);
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(pi * f0 / fs);
    const double a0 = 1.0 + K / Q + K * K;
    out[5] = 1.0f;
    out[6] = -2.0f;
    out[7] = 1.0f;
    out[8] = float(2.0 * (K * K - 1.0) / a0);
    out[9] = float((1.0 - K / Q + K * K) / a0);
  }
}

/* -0.691 + 10 log10 of the mean square of both channels over n blocks; the sums run over the blocks in order, z_l
 * then z_r of each. */
inline double loud_window(const fmd_loud_block* blk, unsigned n, unsigned block_frames)
{
  double sum = 0.0;
  for (unsigned i = 0; i < n; i++)
  {
    sum += double(blk[i].z_l);
    sum += double(blk[i].z_r);
  }
  return -0.691 + 10.0 * std::log10(sum / (double(n) * double(block_frames)));
}

/* BS.1770-4 gating over windows of four consecutive blocks stepping by one.  The power of window w is the sum of its
 * four blocks' (z_l + z_r), blocks in order, over 4 Bf; the means run over the surviving windows in order.  A window
 * whose power is NaN passes no gate (every comparison with it is false). */
inline double loud_integrated(const fmd_loud_block* blk, unsigned n_blocks, unsigned block_frames)
{
  if (n_blocks < 4)
    return -HUGE_VAL;
  std::vector<double> p;
  for (unsigned w = 0; w + 4 <= n_blocks; w++)
  {
    double sum = 0.0;
    for (unsigned i = w; i < w + 4; i++)
      sum += double(blk[i].z_l) + double(blk[i].z_r);
    p.push_back(sum / (4.0 * double(block_frames)));
  }
  const double abs_gate = std::pow(10.0, (-70.0 + 0.691) / 10.0);
  double s1 = 0.0;
  size_t n1 = 0;
  for (double v : p)
    if (v > abs_gate)
    {
      s1 += v;
      n1++;
    }
  if (!n1)
    return -HUGE_VAL;
  const double rel_gate = (s1 / double(n1)) * std::pow(10.0, -10.0 / 10.0);
  double s2 = 0.0;
  size_t n2 = 0;
  for (double v : p)
    if (v > abs_gate && v > rel_gate)
    {
      s2 += v;
      n2++;
    }
  if (!n2)
    return -HUGE_VAL;
  return -0.691 + 10.0 * std::log10(s2 / double(n2));
}

} // namespace fmd
