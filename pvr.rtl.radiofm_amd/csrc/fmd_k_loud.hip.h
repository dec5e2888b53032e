/*
 * fmd_k_loud.hip.h -- the loudness forms of the audio tail (fmd_batch_set_loudness; include/fmd.h, "ITU-R BS.1770
 * loudness blocks"): the eight kernels of fmd_k_tail.hip.h with one argument more, the meter's
 * record.  The same body text (fmd_audio_tail.inc) with FMD_TAIL_LOUD defined: behind every frame the lane takes its
 * float L and R through the two K-weighting biquads, adds the squares to the block's sums and follows the peaks, all
 * in registers; where a block ends inside the call -- the same frame for every lane, so the test is scalar -- it
 * stores the block's record, 16 bytes a lane, into the time-major ring.  Chosen only for calls submitted with the
 * meter on, so the eight kernels of fmd_k_tail.hip.h keep their instructions.
 * Part of fmd_kernels.hip.h for the meter's records and the launch function's declaration; the kernels themselves
 * are compiled where FMD_LOUD_KERNELS is defined: fmd_loud.hip.
 */
#pragma once

#include "fmd_k_tail.hip.h"

namespace fmd
{

/* Rows of the meter's state array [LOUD_STATE_ROWS][CP]: the two delay words of stage 1 (high shelf) and of stage 2
 * (high-pass) for L and R, then the block in progress -- its two sums and two peaks, the rows a call boundary
 * carries (fmd_batch_debug_loud_skip_carry zeroes exactly these four). */
enum LoudRow
{
  LD_S1_1L, LD_S2_1L, LD_S1_1R, LD_S2_1R, // stage 1
  LD_S1_2L, LD_S2_2L, LD_S1_2R, LD_S2_2R, // stage 2
  LD_Z_L, LD_Z_R, LD_PEAK_L, LD_PEAK_R,   // the block in progress
  LOUD_STATE_ROWS
};

/* The meter's part of a loudness tail's argument record.  Everything but the two pointers is the same for every lane
 * of the batch: the host knows at submission where the call's blocks end (all channels tick alike). */
struct LoudArgs
{
  float b0[2], b1[2], b2[2], a1[2], a2[2]; // [stage]: fmd_batch_get_loudness_coeffs
  float* __restrict__ state;               // [LOUD_STATE_ROWS][CP]
  float4* __restrict__ ring;               // [ring_blocks][CP] records { z_l, z_r, peak_l, peak_r }
  unsigned left0;       // frames of this call up to and including the one that ends the block in progress (1 .. Bf)
  unsigned block_frames; // Bf
  unsigned slot0;       // ring row of the block in progress
  unsigned ring_blocks;
};

/* The launch of form (bit 0: S16 audio, bit 1: an audio selection, bit 2: the feed) with the tail's arguments; t0: a
 * profiled call's events around the kernel.  The kernels are instantiated in an object of their own, fmd_loud.hip, so
 * that fmd_batch.o keeps exactly the kernels it had; weak: an fmd_batch.o linked without it never turns the meter on. */
__attribute__((weak, visibility("hidden"))) void loud_tail_launch(
    unsigned form, unsigned CP, hipStream_t s, hipEvent_t t0, hipEvent_t t1, const float2* lp, unsigned A, unsigned C,
    const AudioConsts& k, const ChannelState& st, void* audio, size_t audio_stride, unsigned stereo_q,
    unsigned call_index, unsigned long long* clipped, const int* rows, float* feed_x, const LoudArgs& loud);

#ifdef FMD_LOUD_KERNELS
/* One biquad step in transposed direct form II, every operation rounded on its own (include/fmd.h). */
__device__ __forceinline__ float loud_biquad(float x, float b0, float b1, float b2, float a1, float a2, float& s1,
                                             float& s2)
{
  const float y = __fadd_rn(__fmul_rn(b0, x), s1);
  s1 = __fadd_rn(__fsub_rn(__fmul_rn(b1, x), __fmul_rn(a1, y)), s2);
  s2 = __fsub_rn(__fmul_rn(b2, x), __fmul_rn(a2, y));
  return y;
}

#define FMD_TAIL_LOUD loud
#define FMD_TAIL_COMMON                                                                                               \
  const float2 *__restrict__ lp, unsigned A, unsigned C, unsigned CP, AudioConsts k, ChannelState st

__global__ __launch_bounds__(256) void k_audio_tail_loud(FMD_TAIL_COMMON, float* __restrict__ audio,
                                                        size_t audio_stride, unsigned stereo_q, unsigned call_index,
                                                        LoudArgs loud)
{
  using OUT = OutF32;
#define FMD_TAIL_DONE_ARGS
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_DONE_ARGS
}

__global__ __launch_bounds__(256) void k_audio_tail_s16_loud(FMD_TAIL_COMMON, int16_t* __restrict__ audio,
                                                            size_t audio_stride, unsigned stereo_q,
                                                            unsigned call_index,
                                                            unsigned long long* __restrict__ clipped, LoudArgs loud)
{
  using OUT = OutS16;
#define FMD_TAIL_DONE_ARGS , clipped
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_DONE_ARGS
}

__global__ __launch_bounds__(256) void k_audio_tail_sel_loud(FMD_TAIL_COMMON, float* __restrict__ audio,
                                                            size_t audio_stride, unsigned stereo_q,
                                                            unsigned call_index, const int* __restrict__ rows,
                                                            LoudArgs loud)
{
  using OUT = OutF32;
#define FMD_TAIL_DONE_ARGS
#define FMD_TAIL_ROWS rows
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_ROWS
#undef FMD_TAIL_DONE_ARGS
}

__global__ __launch_bounds__(256) void k_audio_tail_s16_sel_loud(FMD_TAIL_COMMON, int16_t* __restrict__ audio,
                                                                size_t audio_stride, unsigned stereo_q,
                                                                unsigned call_index,
                                                                unsigned long long* __restrict__ clipped,
                                                                const int* __restrict__ rows, LoudArgs loud)
{
  using OUT = OutS16;
#define FMD_TAIL_DONE_ARGS , clipped
#define FMD_TAIL_ROWS rows
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_ROWS
#undef FMD_TAIL_DONE_ARGS
}

#define FMD_TAIL_FEED feed_x
__global__ __launch_bounds__(256) void k_audio_tail_feed_loud(FMD_TAIL_COMMON, float* __restrict__ audio,
                                                             size_t audio_stride, unsigned stereo_q,
                                                             unsigned call_index, float* __restrict__ feed_x,
                                                             LoudArgs loud)
{
  using OUT = OutF32;
#define FMD_TAIL_DONE_ARGS
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_DONE_ARGS
}

__global__ __launch_bounds__(256) void k_audio_tail_s16_feed_loud(FMD_TAIL_COMMON, int16_t* __restrict__ audio,
                                                                 size_t audio_stride, unsigned stereo_q,
                                                                 unsigned call_index,
                                                                 unsigned long long* __restrict__ clipped,
                                                                 float* __restrict__ feed_x, LoudArgs loud)
{
  using OUT = OutS16;
#define FMD_TAIL_DONE_ARGS , clipped
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_DONE_ARGS
}

__global__ __launch_bounds__(256) void k_audio_tail_sel_feed_loud(FMD_TAIL_COMMON, float* __restrict__ audio,
                                                                 size_t audio_stride, unsigned stereo_q,
                                                                 unsigned call_index, const int* __restrict__ rows,
                                                                 float* __restrict__ feed_x, LoudArgs loud)
{
  using OUT = OutF32;
#define FMD_TAIL_DONE_ARGS
#define FMD_TAIL_ROWS rows
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_ROWS
#undef FMD_TAIL_DONE_ARGS
}

__global__ __launch_bounds__(256) void k_audio_tail_s16_sel_feed_loud(FMD_TAIL_COMMON, int16_t* __restrict__ audio,
                                                                     size_t audio_stride, unsigned stereo_q,
                                                                     unsigned call_index,
                                                                     unsigned long long* __restrict__ clipped,
                                                                     const int* __restrict__ rows,
                                                                     float* __restrict__ feed_x, LoudArgs loud)
{
  using OUT = OutS16;
#define FMD_TAIL_DONE_ARGS , clipped
#define FMD_TAIL_ROWS rows
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_ROWS
#undef FMD_TAIL_DONE_ARGS
}
#undef FMD_TAIL_FEED
#undef FMD_TAIL_COMMON
#undef FMD_TAIL_LOUD
#endif // FMD_LOUD_KERNELS

} // namespace fmd
