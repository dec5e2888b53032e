/*
 * fmd_loud.hip -- the loudness forms of the audio tail (k_audio_tail*_loud, fmd_k_loud.hip.h; fmd_batch_set_loudness,
 * include/fmd.h) and their launch, an object of their own in libfmd_hip.so.  The host side -- mode, block bookkeeping,
 * collect -- is in fmd_batch.hip; it reaches these kernels through the function below and nothing else.  Built with
 * fmd_batch.hip's flags.
 */
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#define FMD_TAIL_POLICIES_ONLY // of fmd_k_tail.hip.h: the output policies, not the kernels fmd_batch.o has
#define FMD_LOUD_KERNELS
#include "fmd_k_common.hip.h"
#include "fmd_k_tail.hip.h"
#include "fmd_k_loud.hip.h"

namespace fmd
{

namespace
{

template <typename... P, typename... A>
void launch_tail(void (*kern)(P...), unsigned CP, hipStream_t s, hipEvent_t t0, hipEvent_t t1, A... args)
{
  static_assert(sizeof...(P) == sizeof...(A), "kernel argument count");
  const dim3 grid(CP / 64), block(64, 1);
  if (t0) // (a profiled call: the two events take the kernel's own start and stop)
    hipExtLaunchKernelGGL(kern, grid, block, 0, s, t0, t1, 0u, static_cast<P>(args)...);
  else
    hipLaunchKernelGGL(kern, grid, block, 0, s, static_cast<P>(args)...);
}

} // namespace

void loud_tail_launch(unsigned form, unsigned CP, hipStream_t s, hipEvent_t t0, hipEvent_t t1, const float2* lp,
                      unsigned A, unsigned C, const AudioConsts& k, const ChannelState& st, void* audio,
                      size_t audio_stride, unsigned stereo_q, unsigned call_index, unsigned long long* clipped,
                      const int* rows, float* feed_x, const LoudArgs& loud)
{
  float* const af = static_cast<float*>(audio);
  int16_t* const as = static_cast<int16_t*>(audio);
  auto go = [&](auto kern, auto* a, auto... more) {
    launch_tail(kern, CP, s, t0, t1, lp, A, C, CP, k, st, a, audio_stride, stereo_q, call_index, more..., loud);
  };
  switch (form & 7u)
  {
    case 0:
      return go(k_audio_tail_loud, af);
    case 1:
      return go(k_audio_tail_s16_loud, as, clipped);
    case 2:
      return go(k_audio_tail_sel_loud, af, rows);
    case 3:
      return go(k_audio_tail_s16_sel_loud, as, clipped, rows);
    case 4:
      return go(k_audio_tail_feed_loud, af, feed_x);
    case 5:
      return go(k_audio_tail_s16_feed_loud, as, clipped, feed_x);
    case 6:
      return go(k_audio_tail_sel_feed_loud, af, rows, feed_x);
    default:
      return go(k_audio_tail_s16_sel_feed_loud, as, clipped, rows, feed_x);
  }
}

} // namespace fmd
