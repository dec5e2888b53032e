/*
 * fmd_chan.hip -- the polyphase channeliser's kernels (k_chan / k_chan_roll, fmd_k_chan.hip.h; fmd_chan_*,
 * include/fmd.h) and their launches, an object of their own in libfmd_hip.so.  The host side -- checks, geometry,
 * tables, state -- is fmd_chan.inc.hpp in fmd_batch.hip; it reaches these kernels through the three functions below
 * and nothing else.  Built with fmd_batch.hip's flags.
 */
#include "../../include/fmd.h"

#include "fmd_k_common.hip.h"
#include "fmd_k_chan.hip.h"

namespace fmd
{

namespace
{

template <class In>
hipError_t prepare(unsigned lds)
{
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_chan<In>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             int(lds));
}

template <class In>
void roll(unsigned G, unsigned K, const void* in, size_t in_stride, unsigned n, const float2* hist_in,
          float2* hist_out, hipStream_t stream)
{
  hipLaunchKernelGGL((k_chan_roll<In>), dim3((K + 255) / 256, G), dim3(256), 0, stream, in, in_stride, n, hist_in,
                     hist_out, K);
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
  return int(e);
}

void chan_launch(int format, unsigned ntiles, unsigned G, unsigned lds, hipStream_t stream, const ChanArgs& a)
{
  const dim3 grid(ntiles, G), block(kChanThreads);
  switch (format)
  {
  case FMD_IQ_U8: hipLaunchKernelGGL((k_chan<ChanInU8>), grid, block, lds, stream, a); break;
  case FMD_IQ_S8: hipLaunchKernelGGL((k_chan<ChanInS8>), grid, block, lds, stream, a); break;
  case FMD_IQ_S16: hipLaunchKernelGGL((k_chan<ChanInS16>), grid, block, lds, stream, a); break;
  default: hipLaunchKernelGGL((k_chan<ChanInF32>), grid, block, lds, stream, a); break;
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
  default: roll<ChanInF32>(G, K, in, in_stride, n, hist_in, hist_out, stream); break;
  }
}

} // namespace fmd
