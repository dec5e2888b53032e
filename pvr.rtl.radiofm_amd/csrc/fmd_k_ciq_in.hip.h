/*
 * fmd_k_ciq_in.hip.h -- the channel IQ as an input (FMD_IN_CIQ_*): k_ciq_in copies the caller's rows, float pairs or
 * pairs of 16-bit integers, into the IF stage's channel-major rows `demod` [C][Mstride] float2 -- the mirror of
 * k_ciq_out (fmd_k_ciq.hip.h).  A call with such rows launches it in the IF stage's place (stage_if), through
 * ciq_in_launch: the kernels are instantiated in an object of their own, fmd_ciq_in.hip.
 * Part of fmd_kernels.hip.h (layout, numerics contract and citations: see there and fmd_k_common.hip.h).
 */
#pragma once

#include "fmd_k_common.hip.h"
#include "fmd_k_ciq.hip.h"

namespace fmd
{

/* The load policies of k_ciq_in: the call's `iq_format`.  A lane starts with PER consecutive complex samples of one
 * channel, 16 bytes either way. */
struct InCiqF32
{ // the float2 a call's FMD_CIQ_F32 rows (or FMD_TAP_DEMOD) delivered, as is
  using elem_t = float;
  static constexpr unsigned PER = 2;
};
struct InCiqS16
{ // fmd_ciq16_to_f32 of both parts, host byte order
  using elem_t = int16_t;
  static constexpr unsigned PER = 4;
};

/* The body: workgroup (row, tile) takes CIQ_G consecutive groups of one row, lane i group i of them -- one 16-byte
 * load of the caller's row a lane, one (F32) or two (S16) 16-byte stores into the channel's row of demod, both sides
 * contiguous over the wave.  No transpose, no LDS: the destination is channel-major.
 * src: the input row, on a 16-byte boundary (pointer and stride are the entry point's to check); dst: the channel's
 * row of demod, 128-byte aligned (Mstride is a multiple of 16 samples): every group is aligned on both sides.
 * The row's last, partial group is read and written element by element: nothing is read at or behind sample M of the
 * caller's row (it may end there) and nothing is written at or behind sample M <= Mmax <= Mstride of demod's. */
template <class Fmt>
__device__ __forceinline__ void ciq_in_groups(const typename Fmt::elem_t* __restrict__ src, float2* __restrict__ dst,
                                              unsigned M)
{
  constexpr unsigned PER = Fmt::PER;
  const unsigned k = (blockIdx.y * CIQ_G + threadIdx.x) * PER; // the group's first sample
  if (k >= M)
    return;
  const typename Fmt::elem_t* s = src + 2u * size_t(k);
  float2* o = dst + k;
  const bool whole = k + PER <= M;
  if constexpr (PER == 2)
  {
    if (whole)
      *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(s);
    else
    { // (one sample; volatile: see fmd_mpx_tile.inc -- the compiler otherwise re-fuses and splits such stores)
      volatile float* ov = reinterpret_cast<float*>(o);
      const float re = s[0], im = s[1];
      ov[0] = re;
      ov[1] = im;
    }
  }
  else
  {
    if (whole)
    {
      const uint4 v = *reinterpret_cast<const uint4*>(s);
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
      float x[8];
#pragma unroll
      for (unsigned e = 0; e < 4; e++)
      {
        x[2 * e] = fmd_ciq16_to_f32((int)(w[e] << 16) >> 16);
        x[2 * e + 1] = fmd_ciq16_to_f32((int)w[e] >> 16);
      }
      float4* o4 = reinterpret_cast<float4*>(o);
      o4[0] = make_float4(x[0], x[1], x[2], x[3]);
      o4[1] = make_float4(x[4], x[5], x[6], x[7]);
    }
    else
    {
      volatile float* ov = reinterpret_cast<float*>(o);
#pragma unroll
      for (unsigned e = 0; e < 3; e++)
        if (k + e < M)
        {
          const float re = fmd_ciq16_to_f32(s[2 * e]), im = fmd_ciq16_to_f32(s[2 * e + 1]);
          ov[2 * e] = re;
          ov[2 * e + 1] = im;
        }
    }
  }
}

/* One row per channel: grid (C, tiles of CIQ_G groups), 256 lanes; channel c reads the row at in + c * stride complex
 * samples (stride 0: every channel the same row).  Channels at or above C have no workgroup. */
template <class Fmt>
__global__ __launch_bounds__(256) void k_ciq_in(const typename Fmt::elem_t* __restrict__ in, size_t stride, unsigned M,
                                                float2* __restrict__ demod, unsigned Mstride)
{
  const unsigned c = blockIdx.x;
  ciq_in_groups<Fmt>(in + 2u * size_t(c) * stride, demod + size_t(c) * Mstride, M);
}

/* The kernels live in a translation unit of their own, fmd_ciq_in.hip: it instantiates them and holds the launch
 * below.  fmd_batch.hip's object keeps the kernels it had (tests/test_call_trace_cpu.py links that object alone against
 * a recording double of the runtime and pins its kernel list), so there the launch is a weak reference: in the library
 * it is always present, and a program that links fmd_batch.o without fmd_ciq_in.o has FMD_IN_CIQ_* calls refused,
 * never another kernel.
 * s16: FMD_IN_CIQ_S16, else _F32; grid (C, tiles) of CIQ_G lanes on stream s; t0 / t1: events that take the kernel's
 * own start and stop, or null. */
__attribute__((weak, visibility("hidden"))) void ciq_in_launch(bool s16, unsigned C, unsigned tiles, hipStream_t s,
                                                               hipEvent_t t0, hipEvent_t t1, const void* in,
                                                               size_t stride, unsigned M, float2* demod,
                                                               unsigned Mstride);

} // namespace fmd
