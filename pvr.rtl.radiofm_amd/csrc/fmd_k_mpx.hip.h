/*
 * fmd_k_mpx.hip.h -- the demodulated multiplex (MPX) as an output: k_mpx_out transposes the serial stage's
 * time-major baseband rows into one contiguous row per channel, as float or as 16-bit integers (FMD_MPX_*);
 * k_debug_mpx is the device build of the conversion for fmd_debug_math.
 * Part of fmd_kernels.hip.h (layout, numerics contract and citations: see there and fmd_k_common.hip.h).
 */
#pragma once

#include "fmd_k_common.hip.h"

namespace fmd
{

/* The store policies of k_mpx_out: the call's `mpx_format`.  A lane ends with PER consecutive samples of one
 * channel, 16 bytes either way. */
struct MpxF32
{ // the float the FM PLL left (FmDecode.cpp:433), as is
  using elem_t = float;
  static constexpr unsigned PER = 4;
};
struct MpxS16
{ // fmd_f32_to_mpx16 of it, host byte order
  using elem_t = int16_t;
  static constexpr unsigned PER = 8;
};

constexpr unsigned MPX_T = 64; // time steps of a tile: 256 contiguous bytes of a float row, 128 of an int16 row

/* One workgroup (4 waves) per tile of 64 channels x MPX_T time steps of `in`, the `.x` halves of the float2 rows
 * [t][CP] the serial stage wrote (in = first data row, as floats); out: row c at out + c * stride elements.
 *
 * Reads: wave w takes the tile's rows 16 jj + 4 w + e (jj, e = 0..3), a lane one channel: per row the 64 lanes
 * read the `.x` of 64 consecutive float2 (512 contiguous bytes; rows at or behind M are not read).
 *
 * LDS image (16 KiB): channel-major, a channel's 64 floats are one 256-byte bank row of sixteen 16-byte slots;
 * slot j (time steps 4 j .. 4 j + 3) of channel c lies at slot (j + (c >> 1)) % 16 of row c.
 *   writes  ds_write_b128, one slot a lane (four rows of one channel): bank = (a / 4) % 32, eight consecutive
 *           lanes a cycle.  Lane l holds channel (l & 48) + 2 (l & 7) + ((l >> 3) & 1): the eight lanes of a cycle
 *           hold every second channel, c >> 1 = 8 a + k for k = 0..7, slots (j + k) % 8 -- eight different
 *           slots of the 32 banks: 0 conflicts.
 *   reads   ds_read_b128, bank = (a / 4) % 64, sixteen lanes a cycle ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the
 *           same + 32).  F32: lane l reads slot l & 15 of channel c0 + (l >> 4), c0 a multiple of 4 -- a cycle holds
 *           slots {0-3,12-15} of one channel and {4-11} of its pair (or the other way round): same c >> 1, so the
 *           sixteen slots are the sixteen of a bank row, rotated: 0 conflicts.  S16: lane l reads slots 2 (l & 7)
 *           and 2 (l & 7) + 1 of channel c0 + (l >> 3), c0 a multiple of 8 -- a cycle holds the even (odd) slots
 *           of a pair's two half rows and of the next pair's, rotated by one more: sixteen different slots, 0
 *           conflicts.
 * Stores: 16 bytes a lane; sixteen (F32) / eight (S16) consecutive lanes fill 256 / 128 contiguous bytes of a channel's
 * row.  Rows start on 16-byte boundaries (pointer and stride are the entry point's to check) and a tile starts at a
 * multiple of 64 elements, so every group is aligned.  Channels >= C are not stored; the call's last tile, where it
 * reaches over M, is stored element by element, never at or behind M. */
template <class Fmt>
__global__ __launch_bounds__(256) void k_mpx_out(const float* __restrict__ in, unsigned M, unsigned C, unsigned CP,
                                                 typename Fmt::elem_t* __restrict__ out, size_t stride)
{
  __shared__ __attribute__((aligned(16))) float tile[64 * MPX_T];
  const unsigned l = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const unsigned ch0 = blockIdx.x * 64u, t0 = blockIdx.y * MPX_T;
  {
    const unsigned c = (l & 48u) + 2u * (l & 7u) + ((l >> 3) & 1u);
    const float* src = in + 2u * size_t(ch0 + c);
    float4 v[4];
#pragma unroll
    for (unsigned jj = 0; jj < 4; jj++)
    {
      const unsigned t = t0 + 4u * (w + 4u * jj);
      float x[4];
#pragma unroll
      for (unsigned e = 0; e < 4; e++)
        x[e] = (t + e < M) ? src[2u * size_t(t + e) * CP] : 0.0f;
      v[jj] = make_float4(x[0], x[1], x[2], x[3]);
    }
#pragma unroll
    for (unsigned jj = 0; jj < 4; jj++)
      *reinterpret_cast<float4*>(&tile[c * MPX_T + 4u * ((w + 4u * jj + (c >> 1)) & 15u)]) = v[jj];
  }
  __syncthreads();
  constexpr unsigned PER = Fmt::PER;       // samples a lane stores at a time
  constexpr unsigned LPR = MPX_T / PER;    // lanes per channel row of the tile: 16 / 8
  constexpr unsigned CPI = 64u / LPR;      // channels per wave and read: 4 / 8
  constexpr unsigned NI = 16u / CPI;       // groups of PER samples per lane: 4 / 2
  const unsigned g = l % LPR;              // the lane's group of PER samples in its channels' rows
  const unsigned t = t0 + PER * g;
  float x[NI][PER];
#pragma unroll
  for (unsigned i = 0; i < NI; i++)
  {
    const unsigned c = 16u * w + CPI * i + l / LPR;
#pragma unroll
    for (unsigned s = 0; s < PER / 4u; s++)
    {
      const float4 f =
          *reinterpret_cast<const float4*>(&tile[c * MPX_T + 4u * (((PER / 4u) * g + s + (c >> 1)) & 15u)]);
      x[i][4 * s] = f.x;
      x[i][4 * s + 1] = f.y;
      x[i][4 * s + 2] = f.z;
      x[i][4 * s + 3] = f.w;
    }
  }
  const bool whole = t0 + MPX_T <= M; // (the workgroup's: every tile but the call's last one)
#pragma unroll
  for (unsigned i = 0; i < NI; i++)
  {
    const unsigned c = 16u * w + CPI * i + l / LPR;
    if (ch0 + c >= C)
      continue;
    typename Fmt::elem_t* o = out + size_t(ch0 + c) * stride + t;
    if constexpr (PER == 4)
    {
      if (whole)
        *reinterpret_cast<float4*>(o) = make_float4(x[i][0], x[i][1], x[i][2], x[i][3]);
      else
      { // (volatile: the compiler otherwise folds these stores into the 16-byte one and splits that in 12 + 4)
        volatile float* ov = o;
#pragma unroll
        for (unsigned e = 0; e < 4; e++)
          if (t + e < M)
            ov[e] = x[i][e];
      }
    }
    else
    {
      unsigned h[8];
#pragma unroll
      for (unsigned e = 0; e < 8; e++)
        h[e] = (unsigned)fmd_f32_to_mpx16(x[i][e]) & 0xffffu;
      if (whole)
        *reinterpret_cast<uint4*>(o) =
            make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
      else
      {
        volatile int16_t* ov = o;
#pragma unroll
        for (unsigned e = 0; e < 8; e++)
          if (t + e < M)
            ov[e] = (int16_t)h[e];
      }
    }
  }
}

/* The device build of fmd_f32_to_mpx16 on an array (fmd_debug_math, what = 9): the result as a float. */
__global__ __launch_bounds__(64) void k_debug_mpx(unsigned n, const float* __restrict__ a, float* __restrict__ o0,
                                                  float* __restrict__ o1)
{
  for (unsigned i = blockIdx.x * 64 + threadIdx.x; i < n; i += gridDim.x * 64)
  {
    o0[i] = (float)fmd_f32_to_mpx16(a[i]);
    o1[i] = 0.0f;
  }
}

} // namespace fmd
