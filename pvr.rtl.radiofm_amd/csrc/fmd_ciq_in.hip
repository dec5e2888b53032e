/*
 * fmd_ciq_in.hip -- the kernels that take channel IQ rows as a call's input (k_ciq_in, fmd_k_ciq_in.hip.h;
 * FMD_IN_CIQ_*, include/fmd.h) and their launch, an object of their own in libfmd_hip.so.  The host side -- checks,
 * plan, schedule -- is fmd_batch_process.inc.hpp in fmd_batch.hip; it reaches these kernels through the function below
 * and nothing else.  Built with fmd_batch.hip's flags.
 */
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "fmd_k_common.hip.h"
#include "fmd_k_ciq_in.hip.h"

namespace fmd
{

namespace
{

template <class Fmt>
void launch_in(const dim3& grid, hipStream_t s, hipEvent_t t0, hipEvent_t t1, const void* in, size_t stride, unsigned M,
               float2* demod, unsigned Mstride)
{
  const auto* rows = static_cast<const typename Fmt::elem_t*>(in);
  if (t0) // (a profiled call: the two events take the kernel's own start and stop)
    hipExtLaunchKernelGGL(k_ciq_in<Fmt>, grid, dim3(CIQ_G), 0, s, t0, t1, 0u, rows, stride, M, demod, Mstride);
  else
    hipLaunchKernelGGL(k_ciq_in<Fmt>, grid, dim3(CIQ_G), 0, s, rows, stride, M, demod, Mstride);
}

} // namespace

void ciq_in_launch(bool s16, unsigned C, unsigned tiles, hipStream_t s, hipEvent_t t0, hipEvent_t t1, const void* in,
                   size_t stride, unsigned M, float2* demod, unsigned Mstride)
{
  const dim3 grid(C, tiles);
  if (s16)
    launch_in<InCiqS16>(grid, s, t0, t1, in, stride, M, demod, Mstride);
  else
    launch_in<InCiqF32>(grid, s, t0, t1, in, stride, M, demod, Mstride);
}

} // namespace fmd
