/*
 * fmd_k_tail.hip.h -- audio tail (k_audio_tail), status record, RDS record export, stream probes,
 * device-math test kernel, history rolls.
 * The tail's output policies OutF32 / OutS16 (FMD_PCM_*).
 * Part of fmd_kernels.hip.h (layout, numerics contract and citations: see there and fmd_k_common.hip.h).
 */
#pragma once

#include "fmd_k_common.hip.h"

namespace fmd
{

/* ------------------------------------------------------------------------------------------ */
/* K8: audio tail, one lane per channel: ProcessDeemphasisFilter (FmDecode.cpp:348-359),        */
/*     19 kHz notch cIirFilter::ProcessTwo (IirFilter.cpp:89-105), L/R matrix (:473-499).       */
/* ------------------------------------------------------------------------------------------ */
constexpr int AT_STEPS = 16; // rows in flight per lane (32: slower inside the pipeline, 0.83 against 0.65 ms)

/* What a lane does with the frames of its channel's row: the output format of the call (FMD_PCM_*), a stateless
 * policy like the IF kernels' InF32 / InU8 / InS8 / InS16.  The kernel holds the row pointer (frame_t* o) and the
 * policy's few registers (State).  Every lane take()s frame u of a tile; the lanes that have a channel store() what
 * is due behind frame u of the tile that starts at frame i0 of the row, flush() the ragged last tile of cnt frames
 * and are done() with the call for channel c.  Recurrence, meter and status record are the kernel's and see float
 * samples whatever the policy. */
struct OutF32
{ // interleaved float L, R: one frame (8 B) per store
  using frame_t = float2;
  struct State
  {
  };
  static __device__ __forceinline__ void take(State&, unsigned, float2) {}
  static __device__ __forceinline__ void store(float2* o, State&, unsigned i0, unsigned u, float2 f) { o[i0 + u] = f; }
  static __device__ __forceinline__ void flush(float2*, State&, unsigned, unsigned, bool) {}
  static __device__ __forceinline__ void done(State&, unsigned) {}
};
struct OutS16
{ // interleaved int16 L, R (fmd_f32_to_s16): a frame is one 32-bit word, four of them go out as one 16-byte store.
  // Rows start on 16-byte boundaries (pointer and stride are checked by the entry point) and a tile is 64 bytes, so
  // every group of four is aligned; the ragged tile's last 1-3 frames take an 8- and / or a 4-byte store: nothing is
  // written behind the call's samples.
  using frame_t = unsigned;
  struct State
  {
    unsigned w[4];      // the frames of the group of four being filled
    unsigned nclip = 0; // samples this call saturated
  };
  static __device__ __forceinline__ void take(State& s, unsigned u, float2 f)
  {
    const unsigned l = (unsigned)fmd_f32_to_s16_count(f.x, &s.nclip) & 0xffffu;
    const unsigned r = (unsigned)fmd_f32_to_s16_count(f.y, &s.nclip);
    s.w[u & 3u] = l | (r << 16);
  }
  static __device__ __forceinline__ void store(unsigned* o, State& s, unsigned i0, unsigned u, float2)
  {
    if ((u & 3u) == 3u)
      *reinterpret_cast<uint4*>(o + i0 + u - 3u) = make_uint4(s.w[0], s.w[1], s.w[2], s.w[3]);
  }
  static __device__ __forceinline__ void flush(unsigned* o, State& s, unsigned i0, unsigned cnt, bool active)
  {
    if (!active)
      return;
    const unsigned at = i0 + (cnt & ~3u);
    if (cnt & 2u)
      *reinterpret_cast<uint2*>(o + at) = make_uint2(s.w[0], s.w[1]);
    if (cnt & 1u)
      o[at + (cnt & 2u)] = (cnt & 2u) ? s.w[2] : s.w[0];
  }
  // clipped: [CP] samples saturated so far (fmd_batch_read_pcm_clipped); calls of a batch run their audio tails in
  // order, so the lane owns its channel's word
  static __device__ __forceinline__ void done(State& s, unsigned c, unsigned long long* __restrict__ clipped)
  {
    if (s.nclip)
      clipped[c] += s.nclip;
  }
};

#ifndef FMD_TAIL_POLICIES_ONLY // (fmd_loud.hip takes the policies above and instantiates kernels of its own)
/* One lane per channel.  The channel-major output ([C][stride], what ProcessStream's caller gets) is
 * written by every lane into its own channel's row, one frame (8 B) per store: the 16 stores that
 * fill a 128-byte line follow each other within ~2000 cycles and meet in the L2.  (Until round 4 the
 * frames went through an LDS tile for 64-byte segments per store; the tile's 8.7 KB kept the
 * whole-CU resampler off every CU an audio tail was on, and the stores are not what bounds a
 * lane-per-channel recurrence.)  The status record goes to device memory; k_status_publish takes it
 * to the host.  OUT = OutS16: 16-byte stores of four frames, and the samples it saturated are added to the
 * channel's counter, the one argument more of that form (fmd_batch_read_pcm_clipped).  The two kernels share their
 * body as text (fmd_audio_tail.inc, like the resampler's walks): the float one has the name, the arguments and the
 * instructions it had before there was a second format. */
__global__ __launch_bounds__(256) void k_audio_tail(const float2* __restrict__ lp, unsigned A,
                                                   unsigned C, unsigned CP, AudioConsts k,
                                                   ChannelState st, float* __restrict__ audio,
                                                   size_t audio_stride, unsigned stereo_q,
                                                   unsigned call_index)
{
  using OUT = OutF32;
#define FMD_TAIL_DONE_ARGS
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_DONE_ARGS
}

__global__ __launch_bounds__(256) void k_audio_tail_s16(const float2* __restrict__ lp, unsigned A,
                                                       unsigned C, unsigned CP, AudioConsts k,
                                                       ChannelState st, int16_t* __restrict__ audio,
                                                       size_t audio_stride, unsigned stereo_q,
                                                       unsigned call_index,
                                                       unsigned long long* __restrict__ clipped)
{
  using OUT = OutS16;
#define FMD_TAIL_DONE_ARGS , clipped
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_DONE_ARGS
}

/* The selected forms (fmd_batch_select_audio): row rows[c] of `audio` is channel c's, a channel whose entry is -1
 * delivers nothing -- its lane runs the recurrence, the meter and the status record and skips the stores, the
 * conversion and the clip count.  The same body text; chosen only for calls with a selection. */
__global__ __launch_bounds__(256) void k_audio_tail_sel(const float2* __restrict__ lp, unsigned A, unsigned C,
                                                       unsigned CP, AudioConsts k, ChannelState st,
                                                       float* __restrict__ audio, size_t audio_stride,
                                                       unsigned stereo_q, unsigned call_index,
                                                       const int* __restrict__ rows)
{
  using OUT = OutF32;
#define FMD_TAIL_DONE_ARGS
#define FMD_TAIL_ROWS rows
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_ROWS
#undef FMD_TAIL_DONE_ARGS
}

__global__ __launch_bounds__(256) void k_audio_tail_s16_sel(const float2* __restrict__ lp, unsigned A, unsigned C,
                                                           unsigned CP, AudioConsts k, ChannelState st,
                                                           int16_t* __restrict__ audio, size_t audio_stride,
                                                           unsigned stereo_q, unsigned call_index,
                                                           unsigned long long* __restrict__ clipped,
                                                           const int* __restrict__ rows)
{
  using OUT = OutS16;
#define FMD_TAIL_DONE_ARGS , clipped
#define FMD_TAIL_ROWS rows
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_ROWS
#undef FMD_TAIL_DONE_ARGS
}

/* The feed forms (fmd_batch_set_feed; fmd_k_feed.hip.h): the four kernels above with one argument more, feed_x = the
 * first of the call's rows in the feed's scratch -- every lane that has a channel also stores the frame's mono mix
 * there.  The same body text; chosen only for calls that deliver the feed, so the four above keep their
 * instructions. */
#define FMD_TAIL_FEED feed_x
__global__ __launch_bounds__(256) void k_audio_tail_feed(const float2* __restrict__ lp, unsigned A, unsigned C,
                                                        unsigned CP, AudioConsts k, ChannelState st,
                                                        float* __restrict__ audio, size_t audio_stride,
                                                        unsigned stereo_q, unsigned call_index,
                                                        float* __restrict__ feed_x)
{
  using OUT = OutF32;
#define FMD_TAIL_DONE_ARGS
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_DONE_ARGS
}

__global__ __launch_bounds__(256) void k_audio_tail_s16_feed(const float2* __restrict__ lp, unsigned A, unsigned C,
                                                            unsigned CP, AudioConsts k, ChannelState st,
                                                            int16_t* __restrict__ audio, size_t audio_stride,
                                                            unsigned stereo_q, unsigned call_index,
                                                            unsigned long long* __restrict__ clipped,
                                                            float* __restrict__ feed_x)
{
  using OUT = OutS16;
#define FMD_TAIL_DONE_ARGS , clipped
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_DONE_ARGS
}

__global__ __launch_bounds__(256) void k_audio_tail_sel_feed(const float2* __restrict__ lp, unsigned A, unsigned C,
                                                            unsigned CP, AudioConsts k, ChannelState st,
                                                            float* __restrict__ audio, size_t audio_stride,
                                                            unsigned stereo_q, unsigned call_index,
                                                            const int* __restrict__ rows, float* __restrict__ feed_x)
{
  using OUT = OutF32;
#define FMD_TAIL_DONE_ARGS
#define FMD_TAIL_ROWS rows
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_ROWS
#undef FMD_TAIL_DONE_ARGS
}

__global__ __launch_bounds__(256) void k_audio_tail_s16_sel_feed(const float2* __restrict__ lp, unsigned A, unsigned C,
                                                                unsigned CP, AudioConsts k, ChannelState st,
                                                                int16_t* __restrict__ audio, size_t audio_stride,
                                                                unsigned stereo_q, unsigned call_index,
                                                                unsigned long long* __restrict__ clipped,
                                                                const int* __restrict__ rows,
                                                                float* __restrict__ feed_x)
{
  using OUT = OutS16;
#define FMD_TAIL_DONE_ARGS , clipped
#define FMD_TAIL_ROWS rows
#include "fmd_audio_tail.inc"
#undef FMD_TAIL_ROWS
#undef FMD_TAIL_DONE_ARGS
}
#undef FMD_TAIL_FEED

/* The last kernel of a call: every channel's status record from device memory to the host's snapshot
 * under the per-channel sequence lock (HostStatusWord), a thread per channel -- one kernel of a few
 * waves pays the two system-scope fences, not the latency-bound audio tail. */
__global__ __launch_bounds__(256) void k_status_publish(ChannelState st, unsigned C, unsigned call_index)
{
  const unsigned c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C)
    return;
  const size_t CPs = st.CP;
  unsigned v[HS_WORDS];
#pragma unroll
  for (int w = HS_SEQ_BEGIN + 1; w < HS_SEQ_END; w++)
    v[w] = st.ds[(size_t)w * CPs + c];
  volatile unsigned* h = st.hs + c;
  h[HS_SEQ_BEGIN * CPs] = call_index;
  __threadfence_system();
#pragma unroll
  for (int w = HS_SEQ_BEGIN + 1; w < HS_SEQ_END; w++)
    h[(size_t)w * CPs] = v[w];
  __threadfence_system();
  h[HS_SEQ_END * CPs] = call_index;
}

/* ------------------------------------------------------------------------------------------ */
/* RDS groups of one call's queue -> fixed-size records in device memory (the N > 1 gather of    */
/* bench.py sends them to rank 0 as they are: no host round trip).  Row = 4 x int32:            */
/* channel + 1 + channel_offset, call index, b0 | b1 << 16, b2 | b3 << 16; rows nobody writes    */
/* stay zero (the host zeroes the buffer first).  One workgroup per queue; `cursor` is the      */
/* running row count over the queues drained into the same buffer.  Empties the queue.          */
/* ------------------------------------------------------------------------------------------ */
__global__ __launch_bounds__(256) void k_rds_export(const RdsGroupRec* __restrict__ queue,
                                                    unsigned* __restrict__ queue_count, unsigned queue_cap,
                                                    int4* __restrict__ rec, unsigned cap,
                                                    unsigned* __restrict__ cursor, unsigned channel_offset,
                                                    unsigned* __restrict__ err)
{
  __shared__ unsigned base_s;
  const unsigned n = min(*queue_count, queue_cap);
  if (threadIdx.x == 0)
    base_s = atomicAdd(cursor, n);
  __syncthreads();
  const unsigned base = base_s;
  for (unsigned i = threadIdx.x; i < n; i += blockDim.x)
  {
    const RdsGroupRec r = queue[i];
    if (base + i < cap)
      rec[base + i] = make_int4((int)(r.channel + 1u + channel_offset), (int)r.call_index,
                                (int)((unsigned)r.blocks[0] | ((unsigned)r.blocks[1] << 16)),
                                (int)((unsigned)r.blocks[2] | ((unsigned)r.blocks[3] << 16)));
  }
  __syncthreads();
  if (threadIdx.x == 0)
  {
    if (base + n > cap)
      dev_error(err + 1, DEVERR_RDS_QUEUE_FULL); // more groups than the caller's record buffer holds
    *queue_count = 0;
  }
}

/* ------------------------------------------------------------------------------------------ */
/* Stream probe (fmd_batch_create): one wave that stays busy for `cycles`, and a no-op.         */
/* ------------------------------------------------------------------------------------------ */
__global__ void k_probe_spin(long long cycles, int* sink)
{
  const long long t0 = __builtin_amdgcn_s_memtime();
  int n = 0;
  while (__builtin_amdgcn_s_memtime() - t0 < cycles)
    n++;
  if (sink && n < 0)
    *sink = n;
}
/* One wave that does nothing for `ticks` of the 100 MHz clock (see the post chain's start in
 * fmd_batch.hip). */
__global__ void k_delay(unsigned ticks)
{
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks)
    __builtin_amdgcn_s_sleep(4);
}

__global__ void k_probe_nop(int* sink)
{
  if (sink && threadIdx.x == 12345)
    *sink = 1;
}

/* ------------------------------------------------------------------------------------------ */
/* Test aid: the device builds of the fmd_math.h helpers on arrays of arguments, so their      */
/* device-only code (reciprocal-based division, ballot branches, table forms) can be swept      */
/* against the host libm directly (fmd_debug_math).                                             */
/* ------------------------------------------------------------------------------------------ */
__global__ __launch_bounds__(64) void k_debug_math(int what, unsigned n, const float* __restrict__ a,
                                                   const float* __restrict__ b, float* __restrict__ o0,
                                                   float* __restrict__ o1,
                                                   const double* __restrict__ sctab_g, FmdSincosTab sct,
                                                   const double* __restrict__ sctab256_g)
{
  __shared__ double sctab[2 * FMD_SINCOS_TAB_SIZE];
  __shared__ double sctab256[2 * FMD_SINCOS_P256_SIZE];
  __shared__ float atab[FMD_ATAN_TAB_FLOATS];
  for (unsigned i = threadIdx.x; i < 2 * FMD_SINCOS_TAB_SIZE; i += 64)
    sctab[i] = sctab_g[i];
  for (unsigned i = threadIdx.x; i < 2 * FMD_SINCOS_P256_SIZE; i += 64)
    sctab256[i] = sctab256_g[i];
  if (threadIdx.x == 0)
    fmd_atan_table_fill(atab);
  __syncthreads();
  for (unsigned i = blockIdx.x * 64 + threadIdx.x; i < (n + 63) / 64 * 64; i += gridDim.x * 64)
  { // whole waves stay in the loop: the helpers use wave-wide ballots
    const unsigned k = min(i, n - 1);
    float r0 = 0.0f, r1 = 0.0f;
    switch (what)
    {
      case 0:
        r0 = fmd_atan2f_tab(a[k], b[k], atab);
        break;
      case 1:
        r0 = fmd_atan2f(a[k], b[k]);
        break;
      case 2:
        fmd_sincos_tab(a[k], sctab, sct, &r0, &r1);
        break;
      case 3:
        fmd_sincos_nco(a[k], &r0, &r1);
        break;
      case 4:
        r0 = fmd_div_midrange(a[k], b[k]);
        break;
      case 5:
        r0 = fmd_u8_to_f32((unsigned)a[k]);
        break;
      case 7:
        fmd_sincos_p256(a[k], sctab256, &r0, &r1);
        break;
      default:
        r0 = fmd_rds_arctan2(a[k], b[k]);
    }
    if (i < n)
    {
      o0[i] = r0;
      o1[i] = r1;
    }
  }
}

/* The device build of fmd_f32_to_s16 on an array (fmd_debug_math, what = 8): the result as a float. */
__global__ __launch_bounds__(64) void k_debug_pcm(unsigned n, const float* __restrict__ a, float* __restrict__ o0,
                                                  float* __restrict__ o1)
{
  for (unsigned i = blockIdx.x * 64 + threadIdx.x; i < n; i += gridDim.x * 64)
  {
    o0[i] = (float)fmd_f32_to_s16(a[i]);
    o1[i] = 0.0f;
  }
}

/* ------------------------------------------------------------------------------------------ */
/* history roll: rows [n, n+H) -> [0, H) of a time-major buffer (element size ES floats)        */
/* ------------------------------------------------------------------------------------------ */
/* dst rows [0, H) <- src rows [n, n+H): the last H rows of (history + n new rows).  src == dst
 * for single buffers (then n >= H is required for the row-parallel form), src != dst for the
 * double-buffered ones. */
/* Up to four rolls of float2 buffers in ONE launch (blockIdx.z = job): the history tails of a chain's
 * stages, all due at the chain's end.  Same semantics per job as k_roll. */
struct RollSet
{
  const float2* src[4];
  float2* dst[4];
  unsigned H[4], n[4];
};
__global__ void k_roll_set(RollSet rs, unsigned CP)
{
  const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= CP)
    return;
  const unsigned job = blockIdx.z;
  const float2* src = rs.src[job];
  float2* dst = rs.dst[job];
  const unsigned H = rs.H[job], n = rs.n[job];
  if (n >= H || src != dst)
  {
    for (unsigned r = blockIdx.y; r < H; r += gridDim.y)
      dst[(size_t)r * CP + c] = src[(size_t)(r + n) * CP + c];
  }
  else if (blockIdx.y == 0)
  {
    for (unsigned r = 0; r < H; r++)
      dst[(size_t)r * CP + c] = src[(size_t)(r + n) * CP + c];
  }
}

template <typename T>
__global__ void k_roll(const T* src, T* dst, unsigned H, unsigned n, unsigned CP)
{
  const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= CP)
    return;
  if (n >= H || src != dst)
  { // source and destination rows are disjoint: one row per blockIdx.y
    for (unsigned r = blockIdx.y; r < H; r += gridDim.y)
      dst[(size_t)r * CP + c] = src[(size_t)(r + n) * CP + c];
  }
  else if (blockIdx.y == 0)
  { // overlapping (tiny block): ascending order is safe (destination row r < source row r + n)
    for (unsigned r = 0; r < H; r++)
      dst[(size_t)r * CP + c] = src[(size_t)(r + n) * CP + c];
  }
}
#endif // FMD_TAIL_POLICIES_ONLY

} // namespace fmd
