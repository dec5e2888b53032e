/*
 * fmd_k_ciq.hip.h -- the channel IQ as an output (FMD_CIQ_*): k_ciq_out copies the IF stage's channel-major rows
 * `demod` [C][Mstride] float2 into the caller's rows, as float pairs or as pairs of 16-bit integers; k_ciq_out_sel is
 * the same for the rows of a selection (fmd_batch_select_ciq).
 * Part of fmd_kernels.hip.h (layout, numerics contract and citations: see there and fmd_k_common.hip.h).
 */
#pragma once

#include "fmd_k_common.hip.h"

namespace fmd
{

/* The store policies of k_ciq_out: the call's `ciq.format`.  A lane ends with PER consecutive complex samples of one
 * channel, 16 bytes either way. */
struct CiqF32
{ // the float2 the IF FIR left (m_BufferIF behind cDownsampleFilter::Process), as is
  using elem_t = float;
  static constexpr unsigned PER = 2;
};
struct CiqS16
{ // fmd_f32_to_mpx16 of both parts, host byte order
  using elem_t = int16_t;
  static constexpr unsigned PER = 4;
};

constexpr unsigned CIQ_G = 256; // groups of 16 output bytes per workgroup: 4 KiB of one output row

/* The body of both writers: workgroup (row, tile) takes CIQ_G consecutive groups of one row, lane i group i of them --
 * the 64 lanes of a wave read 1 KiB (F32; S16: 2 KiB, two loads of 16 bytes a lane) of the source row and write 1 KiB
 * of the output row, both contiguous.  No transpose, no LDS: the source is channel-major already.
 * src: the channel's row of demod, 128-byte aligned (Mstride is a multiple of 16 samples); dst: the output row, on a
 * 16-byte boundary (pointer and stride are the entry point's to check), so every group is aligned on both sides.
 * A group's loads stay inside the row's Mstride samples also where the group reaches over M: it starts at a multiple
 * of PER below M <= Mstride, a multiple of 16.  What they read behind M is stale and is never stored: the row's last,
 * partial group goes out element by element, never at or behind M. */
template <class Fmt>
__device__ __forceinline__ void ciq_groups(const float2* __restrict__ src, typename Fmt::elem_t* __restrict__ dst,
                                           unsigned M)
{
  constexpr unsigned PER = Fmt::PER;
  const unsigned k = (blockIdx.y * CIQ_G + threadIdx.x) * PER; // the group's first sample
  if (k >= M)
    return;
  const float4* s = reinterpret_cast<const float4*>(src + k);
  typename Fmt::elem_t* o = dst + 2u * size_t(k);
  const bool whole = k + PER <= M;
  if constexpr (PER == 2)
  {
    const float4 v = s[0];
    if (whole)
      *reinterpret_cast<float4*>(o) = v;
    else
    { // (one sample; volatile: see fmd_mpx_tile.inc -- the compiler otherwise re-fuses and splits such stores)
      volatile float* ov = o;
      ov[0] = v.x;
      ov[1] = v.y;
    }
  }
  else
  {
    const float4 a = s[0], b = s[1];
    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    unsigned h[8];
#pragma unroll
    for (unsigned e = 0; e < 8; e++)
      h[e] = (unsigned)fmd_f32_to_mpx16(x[e]) & 0xffffu;
    if (whole)
      *reinterpret_cast<uint4*>(o) =
          make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    else
    {
      volatile int16_t* ov = o;
#pragma unroll
      for (unsigned e = 0; e < 4; e++)
        if (k + e < M)
        {
          ov[2 * e] = (int16_t)h[2 * e];
          ov[2 * e + 1] = (int16_t)h[2 * e + 1];
        }
    }
  }
}

/* One row per channel: grid (C, tiles of CIQ_G groups), 256 lanes; row c at out + c * stride complex samples.
 * Channels at or above C have no workgroup. */
template <class Fmt>
__global__ __launch_bounds__(256) void k_ciq_out(const float2* __restrict__ demod, unsigned Mstride, unsigned M,
                                                 typename Fmt::elem_t* __restrict__ out, size_t stride)
{
  const unsigned c = blockIdx.x;
  ciq_groups<Fmt>(demod + size_t(c) * Mstride, out + 2u * size_t(c) * stride, M);
}

/* The selected writer (fmd_batch_select_ciq): grid (n, tiles); ent[e] = (channel the entry reads, output row it
 * writes), e < n.  Whole rows either way: a lone channel costs what it costs in k_ciq_out. */
template <class Fmt>
__global__ __launch_bounds__(256) void k_ciq_out_sel(const float2* __restrict__ demod, unsigned Mstride, unsigned M,
                                                     const int2* __restrict__ ent,
                                                     typename Fmt::elem_t* __restrict__ out, size_t stride)
{
  const int2 e = ent[blockIdx.x];
  ciq_groups<Fmt>(demod + size_t(unsigned(e.x)) * Mstride, out + 2u * size_t(unsigned(e.y)) * stride, M);
}

} // namespace fmd
