/*
 * fmd_split_real.hip -- the real forms of the band splitter's kernels (k_split_real / k_split_roll_real,
 * fmd_k_split.hip.h; fmd_split_create_real, include/fmd.h) and their launches, a second object of libfmd_hip.so.  The
 * host side -- checks, geometry, state -- is fmd_split.inc.hpp in fmd_batch.hip; it reaches these kernels through the
 * two functions below and nothing else.  Built with fmd_batch.hip's flags (-ffp-contract=off: nothing fused).
 */
#include "../../include/fmd.h"

#include "fmd_k_common.hip.h"
#include "fmd_k_split.hip.h"

namespace fmd
{

namespace
{

template <class In>
void launch_real(int form, const dim3& grid, unsigned lds, hipStream_t stream, const SplitArgs& a)
{
  const dim3 block(kSplitThreads);
  if (form == 4)
    hipLaunchKernelGGL((k_split_real<In, 4, 32>), grid, block, lds, stream, a);
  else if (form == 8)
    hipLaunchKernelGGL((k_split_real<In, 8, 64>), grid, block, lds, stream, a);
  else
    hipLaunchKernelGGL((k_split_real<In, 0, 0>), grid, block, lds, stream, a);
}

template <class In>
void roll_real(unsigned G, unsigned K, const void* in, size_t in_stride, unsigned N, const float* hist_in,
               float* hist_out, hipStream_t stream)
{
  hipLaunchKernelGGL((k_split_roll_real<In>), dim3((K + 255) / 256, G), dim3(256), 0, stream, in, in_stride, N,
                     hist_in, hist_out, K);
}

} // namespace

void split_real_launch(int format, int form, unsigned ntiles, unsigned G, unsigned lds, hipStream_t stream,
                       const SplitArgs& a)
{
  const dim3 grid(ntiles, G);
  switch (format)
  {
  case FMD_REAL_S8: launch_real<InRealS8>(form, grid, lds, stream, a); break;
  case FMD_REAL_S16: launch_real<InRealS16>(form, grid, lds, stream, a); break;
  default: launch_real<InRealF32>(form, grid, lds, stream, a); break;
  }
}

void split_real_roll(int format, unsigned G, unsigned K, const void* in, size_t in_stride, unsigned N,
                     const float* hist_in, float* hist_out, hipStream_t stream)
{
  switch (format)
  {
  case FMD_REAL_S8: roll_real<InRealS8>(G, K, in, in_stride, N, hist_in, hist_out, stream); break;
  case FMD_REAL_S16: roll_real<InRealS16>(G, K, in, in_stride, N, hist_in, hist_out, stream); break;
  default: roll_real<InRealF32>(G, K, in, in_stride, N, hist_in, hist_out, stream); break;
  }
}

} // namespace fmd
