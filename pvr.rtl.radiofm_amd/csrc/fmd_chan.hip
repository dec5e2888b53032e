/*
 * fmd_chan.hip -- the polyphase channeliser's kernels (k_chan / k_chan_roll and their real forms, fmd_k_chan.hip.h;
 * fmd_chan_*, include/fmd.h) and their launches, an object of their own in libfmd_hip.so.  The host side -- checks,
 * geometry, tables, state -- is fmd_chan.inc.hpp in fmd_batch.hip; it reaches these kernels through the three
 * functions below and nothing else.  Built with fmd_batch.hip's flags.
 */
#include "../../include/fmd.h"

#include "fmd_k_common.hip.h"
#include "fmd_k_chan.hip.h"

namespace fmd
{

namespace
{

hipError_t allow(const void* kernel, unsigned lds)
{
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
}

/* both row formats of one input format */
template <class In>
hipError_t prepare(unsigned lds)
{
  hipError_t e = allow(reinterpret_cast<const void*>(&k_chan<In, false>), lds);
  if (e == hipSuccess)
    e = allow(reinterpret_cast<const void*>(&k_chan<In, true>), lds);
  return e;
}

template <class In>
hipError_t prepare_real(unsigned lds)
{
  hipError_t e = allow(reinterpret_cast<const void*>(&k_chan_real<In, false>), lds);
  if (e == hipSuccess)
    e = allow(reinterpret_cast<const void*>(&k_chan_real<In, true>), lds);
  return e;
}

template <class In>
void launch(bool s16, const dim3& grid, unsigned lds, hipStream_t stream, const ChanArgs& a)
{
  if (s16)
    hipLaunchKernelGGL((k_chan<In, true>), grid, dim3(kChanThreads), lds, stream, a);
  else
    hipLaunchKernelGGL((k_chan<In, false>), grid, dim3(kChanThreads), lds, stream, a);
}

template <class In>
void launch_real(bool s16, const dim3& grid, unsigned lds, hipStream_t stream, const ChanArgs& a)
{
  if (s16)
    hipLaunchKernelGGL((k_chan_real<In, true>), grid, dim3(kChanThreads), lds, stream, a);
  else
    hipLaunchKernelGGL((k_chan_real<In, false>), grid, dim3(kChanThreads), lds, stream, a);
}

template <class In>
void roll(unsigned G, unsigned K, const void* in, size_t in_stride, unsigned n, const float2* hist_in,
          float2* hist_out, hipStream_t stream)
{
  hipLaunchKernelGGL((k_chan_roll<In>), dim3((K + 255) / 256, G), dim3(256), 0, stream, in, in_stride, n, hist_in,
                     hist_out, K);
}

template <class In>
void roll_real(unsigned G, unsigned K, const void* in, size_t in_stride, unsigned n, const float2* hist_in,
               float2* hist_out, hipStream_t stream)
{
  hipLaunchKernelGGL((k_chan_roll_real<In>), dim3((K + 255) / 256, G), dim3(256), 0, stream, in, in_stride, n,
                     reinterpret_cast<const float*>(hist_in), reinterpret_cast<float*>(hist_out), K);
}

} // namespace

/* a tile above 64 KiB of LDS has to be allowed per kernel, once per process and device */
int chan_prepare(unsigned lds_bytes)
{
  hipError_t e = prepare<ChanInF32>(lds_bytes);
  if (e == hipSuccess)
    e = prepare<ChanInU8>(lds_bytes);
  if (e == hipSuccess)
    e = prepare<ChanInS8>(lds_bytes);
  if (e == hipSuccess)
    e = prepare<ChanInS16>(lds_bytes);
  if (e == hipSuccess)
    e = prepare_real<ChanInRealF32>(lds_bytes);
  if (e == hipSuccess)
    e = prepare_real<ChanInRealS8>(lds_bytes);
  if (e == hipSuccess)
    e = prepare_real<ChanInRealS16>(lds_bytes);
  return int(e);
}

void chan_launch(int format, bool s16, unsigned ntiles, unsigned G, unsigned lds, hipStream_t stream,
                 const ChanArgs& a)
{
  const dim3 grid(ntiles, G);
  switch (format)
  {
  case FMD_IQ_U8: launch<ChanInU8>(s16, grid, lds, stream, a); break;
  case FMD_IQ_S8: launch<ChanInS8>(s16, grid, lds, stream, a); break;
  case FMD_IQ_S16: launch<ChanInS16>(s16, grid, lds, stream, a); break;
  case FMD_REAL_F32: launch_real<ChanInRealF32>(s16, grid, lds, stream, a); break;
  case FMD_REAL_S8: launch_real<ChanInRealS8>(s16, grid, lds, stream, a); break;
  case FMD_REAL_S16: launch_real<ChanInRealS16>(s16, grid, lds, stream, a); break;
  default: launch<ChanInF32>(s16, grid, lds, stream, a); break;
  }
}

void chan_roll(int format, unsigned G, unsigned K, const void* in, size_t in_stride, unsigned n, const float2* hist_in,
               float2* hist_out, hipStream_t stream)
{
  switch (format)
  {
  case FMD_IQ_U8: roll<ChanInU8>(G, K, in, in_stride, n, hist_in, hist_out, stream); break;
  case FMD_IQ_S8: roll<ChanInS8>(G, K, in, in_stride, n, hist_in, hist_out, stream); break;
  case FMD_IQ_S16: roll<ChanInS16>(G, K, in, in_stride, n, hist_in, hist_out, stream); break;
  case FMD_REAL_F32: roll_real<ChanInRealF32>(G, K, in, in_stride, n, hist_in, hist_out, stream); break;
  case FMD_REAL_S8: roll_real<ChanInRealS8>(G, K, in, in_stride, n, hist_in, hist_out, stream); break;
  case FMD_REAL_S16: roll_real<ChanInRealS16>(G, K, in, in_stride, n, hist_in, hist_out, stream); break;
  default: roll<ChanInF32>(G, K, in, in_stride, n, hist_in, hist_out, stream); break;
  }
}

} // namespace fmd
