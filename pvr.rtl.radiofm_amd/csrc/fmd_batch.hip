/*
 * fmd_batch.hip -- C ABI (include/fmd.h) of the MI355X FM decoder: device memory, the
 * per-call position plan (host) and the kernel sequence.  gfx950 only, no CPU fallback.
 *
 * Build (the Makefile): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared fmd_batch.hip
 *                       fmd_split_real.hip fmd_ciq_in.hip -o libfmd_hip.so
 */
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "fmd_call_plan.hpp"
#include "fmd_design.hpp"
#include "fmd_groups.hpp"
#include "fmd_kernels.hip.h"
#include "fmd_loud.hpp"
#include "fmd_receiver.hpp"

namespace
{

thread_local std::string g_err;

int fail(int code, const std::string& msg)
{
  g_err = msg;
  return code;
}

#define HIPCHK(expr)                                                                            \
  do                                                                                            \
  {                                                                                             \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return fail(FMD_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));           \
  } while (0)

enum Stage
{
  ST_IF_FIR = 0,
  ST_DEMOD_SERIAL,
  ST_RDS_HALFBAND,
  ST_RDS_LPF,
  ST_RDS_SERIAL,
  ST_RESAMPLE,
  ST_AUDIO_LPF,
  ST_AUDIO_TAIL,
  ST_ROLL,
  ST_COUNT
};
const char* kStageNames[ST_COUNT] = {"if_fir",      "demod_serial", "rds_halfband",
                                     "rds_lpf",     "rds_serial",   "resample",
                                     "audio_lpf",   "audio_tail",   "history_roll"};

/* An owning, move-only buffer of n elements: device memory (DevBuf) or page-locked host memory (HostBuf, with the
 * hipHostMalloc flags of the allocation).  alloc() frees what the buffer holds, then takes max(count, 1) zero-filled
 * elements; it sets n only on success and leaves p == nullptr, n == 0 on failure. */
template <typename T, bool HOST>
struct Buf
{
  T* p = nullptr;
  size_t n = 0;
  Buf() = default;
  Buf(Buf&& o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
  ~Buf() { release(); }
  int alloc(size_t count, unsigned host_flags = hipHostMallocDefault)
  {
    release();
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    void* v = nullptr;
    if ((HOST ? hipHostMalloc(&v, bytes, host_flags) : hipMalloc(&v, bytes)) != hipSuccess)
      return -1;
    p = static_cast<T*>(v);
    if (HOST)
      std::memset(v, 0, bytes);
    else if (hipMemset(v, 0, bytes) != hipSuccess)
    {
      release();
      return -1;
    }
    n = count;
    return 0;
  }
  void release()
  {
    if (p)
      (void)(HOST ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    n = 0;
  }
};
template <typename T>
using DevBuf = Buf<T, false>;
template <typename T>
using HostBuf = Buf<T, true>;

/* An owning, move-only HIP event; converts to hipEvent_t (null until created).  `in_use` is for the events that
 * guard a staging slot or a table used in rotation, and for nothing else (the events of a call's slot and the
 * profiling events are recorded with hipEventRecord and never look at it): record_use() behind the copy or kernel
 * that reads what the event guards, sync_if_in_use() in front of the host's next write -- a guard that was never
 * set has nothing to wait for. */
struct Event
{
  hipEvent_t e = nullptr;
  bool in_use = false;
  Event() = default;
  Event(Event&& o) noexcept : e(std::exchange(o.e, nullptr)), in_use(std::exchange(o.in_use, false)) {}
  ~Event() { release(); }
  hipError_t create(unsigned flags = hipEventDisableTiming)
  {
    release();
    return hipEventCreateWithFlags(&e, flags);
  }
  void release()
  {
    if (e)
      (void)hipEventDestroy(e);
    e = nullptr;
    in_use = false;
  }
  hipError_t record_use(hipStream_t s)
  {
    in_use = true;
    return hipEventRecord(e, s);
  }
  hipError_t sync_if_in_use() const { return in_use ? hipEventSynchronize(e) : hipSuccess; }
  operator hipEvent_t() const { return e; }
};

/* The record queues of a batch with buffers of its own, one per event slot (a call appends to queue[call_index %
 * kSlots] and to nothing else), as the group queues and the block queues both are: the device queues of `cap` records
 * (PER elements of T each), their counts -- contiguous, one copy reads them all --, and the page-locked staging a
 * drain reads them into: the counts and the records arrive by DMA, no staging kernel.  A drain (drain_queues) names
 * the slots it visits in todo[], then takes the two steps between which the caller synchronises the stream. */
constexpr int kSlots = 8;
template <typename T, unsigned PER>
struct SlotQueues
{
  DevBuf<T> queue[kSlots]; // never drained while a call that appends to it is in flight
  DevBuf<unsigned> counts;
  HostBuf<unsigned> h_counts;
  HostBuf<T> h_recs;
  unsigned cap = 0;
  // one drain's: the slots it visits, what it takes from each, their sum, and what the queues could not hold
  int todo[kSlots] = {}, ntodo = 0;
  unsigned cnt[kSlots] = {};
  size_t total = 0;
  uint64_t over = 0;

  unsigned* count(int slot) const { return counts.p + slot; }
  // (two steps, each family in the order it always allocated in: the trace test sees the memsets)
  int alloc_counts() { return counts.alloc(kSlots) | h_counts.alloc(kSlots); }
  int alloc_queues(unsigned records)
  {
    int bad = 0;
    for (int q = 0; q < kSlots && !bad; q++)
      bad |= queue[q].alloc(size_t(PER) * records);
    cap = bad ? 0 : records;
    return bad;
  }
  void release()
  {
    for (auto& q : queue)
      q.release();
    counts.release();
    h_counts.release();
    cap = 0;
  }
  // step 1: the counts on their way to the host (todo[] is the caller's: it knows which slots are due)
  hipError_t fetch_counts(hipStream_t stream)
  {
    return ntodo ? hipMemcpyAsync(h_counts.p, counts.p, kSlots * sizeof(unsigned), hipMemcpyDeviceToHost, stream)
                 : hipSuccess;
  }
  // step 2 (the counts have arrived): the non-empty queues' first `cap` records back to back into h_recs -- grown to
  // hold at least `grow` records --, their counts cleared.  -1: the staging could not grow.
  int fetch_records(size_t grow, hipStream_t stream)
  {
    total = 0;
    over = 0;
    for (int i = 0; i < ntodo; i++)
    {
      const unsigned n = h_counts.p[todo[i]];
      cnt[i] = std::min(n, cap);
      over += n - cnt[i];
      total += cnt[i];
    }
    if (PER * total > h_recs.n && h_recs.alloc(PER * std::max(total, grow)))
      return -1;
    size_t at = 0;
    for (int i = 0; i < ntodo; i++)
      if (cnt[i])
      {
        if (hipMemcpyAsync(h_recs.p + PER * at, queue[todo[i]].p, size_t(cnt[i]) * PER * sizeof(T), hipMemcpyDeviceToHost,
                           stream) != hipSuccess ||
            hipMemsetAsync(count(todo[i]), 0, sizeof(unsigned), stream) != hipSuccess)
          return -2;
        at += cnt[i];
      }
    return 0;
  }
};

/* One launch of a kernel the profiler can time: with ev_start, hipExtLaunchKernelGGL records ev_start / ev_stop at
 * the kernel's own start and stop (a recorded event would also count the dispatch gap behind it); without, a plain
 * launch.  Every argument is converted to the kernel's parameter type. */
template <typename... P, typename... A>
void launch(void (*kern)(P...), dim3 grid, dim3 block, unsigned lds, hipStream_t s, hipEvent_t ev_start,
            hipEvent_t ev_stop, A... args)
{
  static_assert(sizeof...(P) == sizeof...(A), "kernel argument count");
  if (ev_start)
    hipExtLaunchKernelGGL(kern, grid, block, lds, s, ev_start, ev_stop, 0u, static_cast<P>(args)...);
  else
    hipLaunchKernelGGL(kern, grid, block, lds, s, static_cast<P>(args)...);
}

enum IqFormat
{
  IQ_F32 = 0, // complex<float>, the ProcessStream argument (FmDecode.h:135)
  IQ_U8 = 1,  // RTL-SDR byte pairs, converted like ReadAsyncCB (RTL_SDR_Source.cpp:207-211)
  IQ_S8 = 2,  // signed 8-bit pairs, v * 2^-7 (fmd_s8_to_f32)
  IQ_S16 = 3  // signed 16-bit pairs in host byte order, v * 2^-15 (fmd_s16_to_f32)
};
static_assert(IQ_F32 == FMD_IQ_F32 && IQ_U8 == FMD_IQ_U8 && IQ_S8 == FMD_IQ_S8 && IQ_S16 == FMD_IQ_S16,
              "the plan's formats are the C ABI's");

/* The format arguments of the C ABI (FMD_IQ_*, FMD_PCM_*, FMD_MPX_*, FMD_FEED_*, FMD_CIQ_*): the values each takes
 * (0 .. last), the bytes of an element -- an IQ sample, one audio, multiplex or feed sample, a complex sample of the
 * channel IQ -- and what a refusal says. */
enum FormatKind { FMT_IQ, FMT_PCM, FMT_MPX, FMT_FEED, FMT_CIQ, FMT_KINDS };
/* a call's four outputs (what fmd_batch::sel and Call::kOut are indexed by) */
constexpr FormatKind kOutKinds[4] = {FMT_PCM, FMT_MPX, FMT_FEED, FMT_CIQ};
struct FormatInfo
{
  int last;
  unsigned char esz[4];
  const char* must;
};
const FormatInfo kFormats[5] = {
    {FMD_IQ_S16, {8, 2, 2, 4}, "iq_format must be one of FMD_IQ_F32, _U8, _S8, _S16 (0..3)"},
    {FMD_PCM_S16, {4, 2}, "pcm_format must be FMD_PCM_F32 or FMD_PCM_S16 (0..1)"},
    {FMD_MPX_S16, {4, 2}, "mpx_format must be FMD_MPX_F32 or FMD_MPX_S16 (0..1)"},
    {FMD_FEED_S16, {4, 2}, "feed_format must be FMD_FEED_F32 or FMD_FEED_S16 (0..1)"},
    {FMD_CIQ_S16, {8, 4}, "ciq.format must be FMD_CIQ_F32 or FMD_CIQ_S16 (0..1)"}};

/* a format argument, checked before anything else is touched */
inline bool format_ok(FormatKind k, int format)
{
  return format >= 0 && format <= kFormats[k].last;
}

inline size_t format_esz(FormatKind k, int format)
{
  return kFormats[k].esz[format];
}

/* FMD_REAL_* (16 | FMD_IQ_F32, _S8, _S16; no unsigned bytes): real samples, one element each.  Only a real band
 * splitter takes them -- format_ok(FMT_IQ, ..) keeps refusing them everywhere else. */
static_assert(FMD_REAL_F32 == (16 | FMD_IQ_F32) && FMD_REAL_S8 == (16 | FMD_IQ_S8) && FMD_REAL_S16 == (16 | FMD_IQ_S16),
              "a real format is its IQ format with bit 4 set");
inline bool real_format_ok(int format)
{
  return format == FMD_REAL_F32 || format == FMD_REAL_S8 || format == FMD_REAL_S16;
}

inline size_t real_format_esz(int format)
{
  return kFormats[FMT_IQ].esz[format & 3] / 2;
}

/* FMD_IN_CIQ_* (32 | FMD_CIQ_F32, _S16): channel IQ rows as a call's input, the samples behind the IF stage.  Only the
 * _call entry points take them -- format_ok(FMT_IQ, ..) keeps refusing them everywhere else. */
static_assert(FMD_IN_CIQ_F32 == (32 | FMD_CIQ_F32) && FMD_IN_CIQ_S16 == (32 | FMD_CIQ_S16),
              "a channel-IQ input format is its output format with bit 5 set");
inline bool ciq_in_format(int format)
{
  return format == FMD_IN_CIQ_F32 || format == FMD_IN_CIQ_S16;
}
const char* const kCiqInOnlyCall =
    "FMD_IN_CIQ_F32 / _S16 (channel IQ rows as input) are taken by the _call entry points only "
    "(fmd_batch_process_device_call, fmd_batch_process_host_call, fmd_process_stream_call)";

/* Where a call delivers one of its outputs -- the audio, the multiplex (the _mpx entry points), the feed (the _feed
 * entry points), the channel IQ (the _call entry points; its elements are complex samples); p == null: nowhere -- the call launches what a call without the argument launches (and the feed's
 * frame count does not advance). */
struct Out
{
  FormatKind kind;
  void* p = nullptr;       // rows of the format, channel c at p + c * stride elements
  int fmt = 0;             // FMD_PCM_* / FMD_MPX_* / FMD_FEED_* / FMD_CIQ_*
  size_t stride = 0;       // elements
  unsigned* out = nullptr; // (host, optional) elements per row the call wrote
  bool deliver = true;     // false: a feed selection of no rows -- the scratch and the count advance, nothing is written
  size_t esz() const { return format_esz(kind, fmt); }
  // a lane stores 16 bytes of a row at a time: every row has to start on a 16-byte boundary
  bool rows_aligned() const { return !(reinterpret_cast<uintptr_t>(p) % 16) && !(stride % (16 / esz())); }
  // (the rows of the sub-batch that starts at channel ch0: ch0 * stride elements of the output format on; with a
  // selection every sub-batch writes into the one compact output, its table holds global row numbers)
  Out from_channel(unsigned ch0, bool selection) const
  {
    Out o = *this;
    if (p && !selection)
      o.p = static_cast<char*>(p) + size_t(ch0) * stride * esz();
    return o;
  }
};

/* One call of a batch: the input rows, the four outputs, the caller's stream. */
struct Call
{
  const void* iq = nullptr;
  int iq_fmt = FMD_IQ_F32; // FMD_IQ_*; from a call record also FMD_IN_CIQ_*
  size_t iq_stride = 0;    // IQ samples between the input rows
  unsigned samples = 0;    // (FMD_IN_CIQ_*: the call's baseband length M)
  bool from_record = false; // a _call entry point's: the only ones that take FMD_IN_CIQ_*
  bool ciq_in() const { return ciq_in_format(iq_fmt); }
  // bytes of an input sample
  size_t in_esz() const { return ciq_in() ? format_esz(FMT_CIQ, iq_fmt & 1) : format_esz(FMT_IQ, iq_fmt); }
  Out audio{FMT_PCM}, mpx{FMT_MPX}, feed{FMT_FEED}, ciq{FMT_CIQ};
  void* stream = nullptr;
  static constexpr Out Call::* kOut[FMT_KINDS] = {nullptr, &Call::audio, &Call::mpx, &Call::feed, &Call::ciq};
  Out& out(FormatKind k) { return this->*kOut[k]; }
  const Out& out(FormatKind k) const { return this->*kOut[k]; }
};

} // namespace

struct fmd_batch
{
  fmd::Params params;
  fmd::Design des;
  unsigned C = 0, CP = 0;
  int device = 0;
  fmd_callbacks cb{};
  void* user = nullptr;
  std::vector<int> shifts;

  static constexpr int NSLOT = kSlots; // event sets, RDS queues and staging slots in rotation (call_index % NSLOT)

  // host-tracked, batch-uniform positions
  unsigned if_pos = 0;     // cDownsampleFilter::m_pos_int
  unsigned lut_idx = 0;    // cFineTuner::m_index
  float rs_pos = 0.0f;     // cDownsampleFilter::m_pos_frac (mono == stereo)
  unsigned rds_lpf_g = 0;  // samples since init of the RDS LPF, mod taps
  unsigned mf_g = 0;       // samples since init of the RDS matched filter, mod taps
  unsigned alpf_g = 0;     // samples since init of the audio LPF, mod taps
  int hist_sel = 0;        // IF history ping-pong
  uint32_t call_index = 0;

  // geometry
  unsigned min_samples = 0; // smallest call this geometry takes (fmd_batch_min_samples)
  int streams_sharing = 0;  // internal streams the create-time probe found sharing a hardware queue
  unsigned cpc = 1;         // channels per capture (fmd_batch_set_channels_per_capture): channel c reads capture c / cpc
  unsigned Mmax = 0, Mstride = 0, Amax = 0, Rmax = 0;
  std::vector<unsigned> hb_nmax; // max input length per HB stage
  // last call
  unsigned lastM = 0, lastA = 0, lastR = 0;

  // device memory
  DevBuf<float2> lut, hist[2], demod[2], br[2], mix[2], rdsraw[2], rlpf[2], rs[2], alp[2];
  std::vector<DevBuf<float2>> hbbuf; // input buffers of stages 1..n-1 (stage 0 reads mix)
  DevBuf<float> if_coeff, rs_coeff, rds_lpf_taps, mf_taps2, audio_taps, ktab;
  DevBuf<float> rpll, rmf, tap_sync;
  DevBuf<double> sctab, sctab256; // fmd_sincos_tab / fmd_sincos_p256 (the serial stage's two NCOs)
  DevBuf<int> pidx;
  static constexpr unsigned kBrFront = 32; // rows of zeros in front of the history rows (both resamplers reach below)
  float2* brp(int q) const { return br[q].p + size_t(kBrFront) * CP; } // first history row of br[q]
  unsigned rs_margin = 0, rs_row = 0; // ktab: zero entries around each output's taps, row length
  // k_resample_ring (large batches): outputs per wave (0 = this geometry does not fit the CU's LDS),
  // ring batches, batches per group in the tap table, row offset; plan buffers; -1 auto / 0 off / 1 on
  int rsr_R = 0, rsr_NW = 0;
  unsigned rsr_nbr = 0, rsr_nbm = 0;
  int rsr_rb = 0;
  DevBuf<float> rsr_tab;
  DevBuf<int> rsr_head, rsr_steps;
  int rsr_mode = -1;
  int n_cus = 256;
  // k_halfband_chain (large batches, the usual three-stage chains): step lists by (inputs, stretches),
  // uploaded the first time a call size is seen; the stages' last outputs on their way to the history
  // rows; -1 auto / 0 off / 1 on
  struct HbfPlan
  {
    unsigned n_in = 0, S = 0;
    DevBuf<fmd::HbStep> steps;
    DevBuf<int> seg_first;
  };
  std::vector<std::unique_ptr<HbfPlan>> hbf_plans;
  DevBuf<float2> hbf_tail1, hbf_tail2;
  int hbf_mode = -1;
  /* The RDS oscillator (CRDSDownConvert::ProcessData, DownConvert.cpp:436-442) as one sequence per batch,
   * for calls whose serial stage writes no mixed rows (k_demod_serial<.., MIX = false> +
   * k_halfband_chain<.., OSC>): a recurrence on its own state with an amplitude servo, independent of the
   * signal, started at (1, 0) in every decoder and advanced by every baseband sample.  The HOST computes a
   * call's M values while it submits the call (~60 us of one core; a lone GPU wave takes 0.37 ms for the
   * same dependent chain, on a stream the IF FIR needs), in page-locked staging (8 slots) that an
   * asynchronous copy takes to the device tables (4 in rotation: a call's table is read by its half-band
   * chain, two serial stages later), kOscH entries of history in front.  osc_on: every call (large batches
   * from creation; "halfband_chain" = 1 before the first call). */
  static constexpr unsigned kOscH = 64;
  DevBuf<fmd::HbOsc> osc_tab[4]; // (+ HBF_SLACK entries that are read but never used, see k_halfband_chain)
  HostBuf<fmd::HbOsc> h_osc;     // [NSLOT][kOscH + Mmax + 8]
  Event osc_ev[NSLOT];           // behind the copy out of a staging slot
  size_t h_osc_stride = 0;
  float osc_re = 1.0f, osc_im = 0.0f; // CRDSDownConvert: m_Osc1 = (1, 0) (DownConvert.cpp:284)
  bool osc_on = false;
  int dbg_nomix = 1;
  // development switches (fmd_batch_debug_set; the library reads no environment variable)
  int dbg_fir_nt = 0;          // tiles per IF FIR workgroup (0: the library decides)
  int dbg_serial_claim = 0;    // whole-CU serial stage: every role wave claims its SIMD's register file
  int dbg_hb4 = 1, dbg_ring4 = 1; // 0: the generic half-band / ring-FIR kernels where the unrolled ones would run
  int dbg_fir_ro = 2;          // outputs per lane of the headline IF FIR form: 1 k_if_fir_mt, 2 / 3 k_if_fir_mt3
                               // (2: 288 600 MS/s and the FIR 0.975 ms inside the pipeline; 3: 287 500 and 1.00)
  bool dbg_fir_interior = true; // k_if_fir_mt3<.., 2>: tiles inside a call take the interior body ("fir_ro" -2: none
                               // does; the sign of that key and not a key of its own: the key table is held to 14)
  int dbg_lpf_late = -1;       // stream layout of an overlapped call (submit_overlapped): -1 the library decides,
                               // 0 low-pass filters on the heavy stream, 1 on a stream of their own, 2 at the
                               // heads of the light part's two streams
  // where a host-buffer call's time goes (fmd_batch_debug_host_ms): copy in, submission, wait + copy
  // out, RDS collection + group decoder callbacks; sums since the last query
  double host_ms[4] = {0, 0, 0, 0};
  unsigned host_calls = 0;
  DevBuf<long long> serial_probe; // FMD_SERIAL_PROBE=1: per-workgroup timing of the serial stage
  int dbg_stage_mask = 63;        // energy experiment: parts of a call that are launched (63 = all; else wrong results)
  DevBuf<float> fstate; // all float state arrays, CP each
  DevBuf<int> istate;
  DevBuf<uint16_t> r_data;
  SlotQueues<fmd::RdsGroupRec, 1> groups; // the RDS groups of the calls (fmd_batch_collect_rds / _export_rds_device)
  // call whose groups were last taken out of the slot's queue (collect / export): a slot is not
  // visited again before a newer call has used it
  uint32_t drained_call[NSLOT] = {};
  /* The block observation (fmd_batch_set_rds_blocks).  The mode is the caller-facing batch's
   * and every sub-batch's next call's; a call reads it when it is submitted.  Nothing of this exists on the device
   * until the first call of fmd_batch_set_rds_blocks that enables a mode: then the counters ([RQ_N][CP], zero, and
   * from there on touched by nothing but the observing kernels), and with the first mode 2 the block queues -- one
   * per event slot like the group queues, with drained bookkeeping of their own: the two drains are independent. */
  int rb_mode = 0;
  DevBuf<unsigned> rb_quality;         // [RQ_N][CP]
  SlotQueues<uint4, 2> blocks;         // two uint4 per record; blocks.cap is fixed by the first mode 2
  // A mode-2 call has used the slot's queue since it was last drained.  A slot's age is its NEWEST call's
  // (slot_call), whatever that call's mode: records left in a queue for NSLOT calls or more are delivered once the
  // call that has since reused the slot is `lag` calls old -- later than their own call's age would allow, never
  // earlier than a call that may still append.  Collecting at least every NSLOT calls never meets this.
  bool rb_dirty[NSLOT] = {};
  // fmd_batch_export_rds_device drains a queue asynchronously on the caller's stream: the event tells
  // the next call that appends to the same queue (NSLOT calls later) when it is empty
  Event ev_drained[NSLOT];
  bool drained_pending[NSLOT] = {};
  // running row count of one export (k_rds_export): a cursor per call out of a ring, so that two exports
  // on different streams never share one
  static constexpr unsigned kExportCursors = 16;
  DevBuf<unsigned> export_cursor;
  unsigned export_seq = 0;
  fmd::ChannelState st{};
  std::vector<fmd::HbCoef> hbcoef;
  fmd::HbChainTaps hb_taps{}; // the same taps as k_halfband_chain takes them (three-stage chains)

  // device staging of the host-buffer entry points, by kind: the input rows ([FMT_IQ]) and every output's rows (sized
  // on first use, in bytes of the call's format)
  DevBuf<float> h_stage[FMT_KINDS];
  // fmd_batch_debug_mpx_ms (its first query switches this on): the multiplex writer's own start and stop of the last
  // NSLOT calls that asked for the multiplex (events of their own, no slot of the stage list or the timeline)
  int dbg_mpx_timing = 0;
  Event mpx_ev[NSLOT][2]; // (in_use of [slot][0]: a timed launch of the writer has recorded the pair)
  // per channel: audio samples that FMD_PCM_S16 calls saturated since the batch was created (k_audio_tail<OutS16>;
  // fmd_batch_read_pcm_clipped).  It belongs to the output like the audio meter: nothing resets it.
  DevBuf<unsigned long long> pcm_clip; // [CP]

  /* Which channels deliver audio / multiplex rows (fmd_batch_select_audio / _mpx).  The
   * caller-facing batch holds the list as the caller gave it (global channels, row i = list[i]); a batch with buffers
   * of its own holds its part as (local channel, global row) entries sorted by channel, and the row tables its
   * kernels read.  A table is a per-call resource: the audio tail and the multiplex writer run on different streams,
   * and calls in flight keep the selection they were submitted with.  So every change makes a new VERSION -- device
   * table, page-locked staging and an event of its own --, uploaded on the reading kernel's stream right in front of
   * the first kernel that reads it; `read` is recorded behind every reader, and a version is written again only once
   * it is no longer the current one and `read` has completed: behind its last reader.  No call waits for another. */
  struct SelTable
  {
    DevBuf<int> d;      // audio: [CP] output row of every channel, -1 none; multiplex: [C] int2 (channel, row)
    HostBuf<int> h;     // what the upload reads: the version's own, rewritten only with the version
    Event read;         // behind the last kernel that reads d (and so behind the upload)
    hipStream_t stream = nullptr; // where `read` was last recorded
  };
  struct Selection
  {
    bool on = false;              // false: one row per channel, the kernels and launches of a batch without this
    unsigned n_total = 0;         // rows of the whole selection (the caller-facing batch's list)
    std::vector<unsigned> list;   // caller-facing batch: the channels in row order
    std::vector<int2> ent;        // batch with buffers: its part, sorted by channel
    bool dirty = false;           // ent changed since the current version was built
    std::vector<std::unique_ptr<SelTable>> pool;
    int cur = -1;
  };
  Selection sel[FMT_KINDS]; // by output kind (kOutKinds; [FMT_IQ] is never used); feed and channel IQ: the multiplex's form
  /* The mono feed at sample_rate_pcm / feed_div (fmd_batch_set_feed).  Every batch knows the
   * divisor; the caller-facing one keeps the taps for fmd_batch_get_feed_taps.  A batch with buffers of its own holds
   * the taps on the device, the time-major scratch of mono frames -- [feed_T - 1 + Amax][CP] floats: the history rows
   * in front of a call's rows, rolled behind every call that asked for the feed -- and feed_g, the frames of those
   * calls so far: a call's first output and its sample count follow from it on the host, at submission.  One scratch,
   * not two by call parity: a batch's audio tails run in submission order on one stream (the channel state and the
   * clip counter rely on the same); should the stream ever differ from the last feed call's, the tail first waits for
   * feed_done, recorded behind that call's roll.  The feed belongs to the output: resets, retunes, capture switches,
   * imports and loads leave all of this alone. */
  unsigned feed_div = 0, feed_T = 0;
  uint64_t feed_g = 0;
  std::vector<float> feed_taps_h;
  DevBuf<float> feed_taps, feed_x;
  Event feed_done;
  hipStream_t feed_stream = nullptr;
  int dbg_feed_skip_roll = 0;     // fmd_batch_debug_feed_skip_roll (mutation test): the history rows stay stale
  int dbg_ciq_in_skip = 0;        // fmd_batch_debug_ciq_in_skip_tile (mutation test): the input copy's last tile is left out
  /* The loudness meter (fmd_batch_set_loudness).  Every batch knows the mode of its next
   * call, the block length, the ring's rows and the ten coefficients.  A batch with buffers of its own holds the
   * meter's state ([LOUD_STATE_ROWS][CP], +0 at the first mode-1 setting), the time-major ring of block records and
   * loud_g, the frames of its mode-1 calls so far: where a call's blocks end follows from it on the host, at
   * submission -- all channels tick alike.  loud_done[k]: blocks completed by the calls at least k calls old (shifted
   * by every call, whatever its mode), what a lagged collect may take.  The caller-facing batch holds loud_taken, the
   * blocks collected or counted lost so far.  The meter belongs to the output: resets, retunes, capture switches,
   * imports and loads leave all of this alone. */
  int loud_mode = 0;
  unsigned loud_bf = 0, loud_ring = 0;
  float loud_coef[10] = {};
  DevBuf<float> loud_state;
  DevBuf<float4> loud_blocks;
  uint64_t loud_g = 0, loud_done[5] = {}, loud_taken = 0;
  int dbg_loud_skip_carry = 0;    // fmd_batch_debug_loud_skip_carry (mutation test): a call starts its block from +0
  /* The channel IQ (the _call entry points): demod[q]'s rows as an output.  It has no state
   * of its own -- a selection of the multiplex's form (sel[FMT_CIQ]) and the host call's staging. */
  bool decoder_owned = false;     // the one-channel batch behind an fmd_decoder: it takes no selection

  std::vector<std::unique_ptr<fmd::GroupDecoder>> gdec;

  // profiling: 0 off, 1 = events around the IF FIR kernel only, 2 = around every stage.
  // One event set per call (up to kMaxProfCalls) so nothing has to synchronise inside a timed loop.
  int profiling = 0;
  int write_taps = 0; // stage taps of the RDS recurrences are only written on request

  // Internal streams: the IF FIR of the next calls (s_fir), the serial stage of this call (s_ser), the heavy part of
  // the post chain behind it (s_post: half-band chain, resampler) and its light part (s_rds, s_lpf: see the stream
  // layouts in front of submit_overlapped; a batch of one or two wavefronts runs its RDS chain and its audio chain side by
  // side on s_rds / s_post) are independent chains tied together, and to the caller's stream, with events.  Streams
  // of their own on purpose, and picked by measurement (pick_independent_streams): HIP multiplexes streams onto a
  // few hardware queues and two chains sharing a queue block each other.  demod, br, mix and the filters' inputs
  // are double-buffered by call parity so no chain waits on a buffer a younger call still reads.
  //   concurrency 0: everything on the caller's stream (also forced by profiling level 2)
  //   concurrency 1: internal streams, the caller's stream is ordered after every call (default)
  //   concurrency 2: as 1, but the caller's stream is only ordered after a call by fmd_batch_wait /
  //                  fmd_batch_collect_rds; lets call k+1's FIR overlap call k's serial stages
  int concurrency = 1;
  hipStream_t s_fir = nullptr, s_ser = nullptr, s_post = nullptr, s_rds = nullptr, s_lpf = nullptr;
  /* More channels than the whole-CU pipeline is built for (kSubBatchChannels = 64 CUs' worth of serial stage): the
   * batch the caller holds is a SHELL over ceil(C / 8192) sub-batches of equal size, each a complete batch of its own
   * (buffers, channel state, RDS queues, status snapshot), all on the shell's five streams.  A call is submitted
   * sub-batch by sub-batch, so that on the streams the sub-batch calls form ONE sequence of 8192-channel calls --
   * FIR(k, s + 1) behind heavy(k, s - 1), serial stages back to back -- i.e. the pipeline DESIGN.md section 2
   * describes, at its rate, whatever C is (channels are independent: FmDecode.h:201-212).  The shell owns the
   * streams, the caller-facing bookkeeping (group decoders, host staging, export cursor) and nothing on the device. */
  std::vector<std::unique_ptr<fmd_batch>> subs;
  std::vector<unsigned> sub_ch0;   // first channel of every sub-batch, and C behind the last
  bool owns_streams = true;        // false: a sub-batch, the streams are its shell's
  hipEvent_t vheavy[2] = {nullptr, nullptr}; // shell: EV_HEAVY of the last two sub-batch calls of the common sequence
  // sub-batch: EV_HEAVY of the sub-batch call two back in the common sequence -- this call's IF FIR stays behind it
  // (submit_front); else null
  hipEvent_t sched_prev2 = nullptr;
  bool split_post = false;
  bool serial_exclusive = false; // serial stage owns whole CUs (small batches, see the launch)
  enum { EV_IN, EV_FIR, EV_INDONE, EV_SER, EV_AUD, EV_RDS, EV_HEAVY, EV_RDSH, EV_ALP, EV_DEC, EV_ROLL, EV_N };
  Event cev[NSLOT][EV_N];
  uint32_t slot_call[NSLOT] = {}; // call index that last used the slot (0 = never)
  std::vector<Event> ev; // [calls][ST_COUNT + 1]
  unsigned prof_calls = 0;

  // Device-side error word (fmd::DevErr bits) in host-mapped memory: kernels OR into it, the host
  // reads it without a copy or a synchronisation.  `failed`: a call broke off after its first launch
  // or a kernel reported an error -- the channel state is no longer trustworthy, every later call is
  // refused until fmd_batch_reset / destroy.
  HostBuf<unsigned> h_err; // [0] fatal bits, [1] recoverable ones (groups lost), see fmd::DevErr
  bool failed = false;
  std::string fail_msg;
  unsigned spin_limit = 1u << 20; // fmd_batch_debug_set_spin_limit
  bool if_dry_run = false;        // launch_if_stage stops behind its feasibility checks
  // Status snapshot in host-mapped memory, written by the last kernel of every call
  // (fmd::HostStatusWord): what the getters read -- no device call, no batch bookkeeping touched,
  // so they are safe from any thread while another one is inside a process call.
  HostBuf<unsigned> h_status;
  DevBuf<unsigned> d_status; // the same record in device memory: what the kernels write (k_status_publish copies)
  unsigned host_seq = 0; // tags of snapshot updates made by the host (create, reset)

  /* Retuning single channels (fmd_batch_enable_retune / fmd_batch_retune_channels).
   * The caller-facing batch (plain or shell) owns the silent twin -- a one-channel batch of the same geometry on
   * the same streams, fed zeros of every call's size and reset with the batch -- and the per-channel log of
   * shift changes (status getters, group decoders).  A batch with buffers of its own (plain or sub-batch) holds
   * the edits its next call applies and what k_channel_restart needs to apply them. */
  fmd_params cparams{};                // the create arguments (the twin is made from them)
  std::unique_ptr<fmd_batch> twin;
  DevBuf<float2> twin_iq;              // FMD_MAX_BLOCK zeros
  DevBuf<float> twin_audio;
  std::mutex log_mu;                   // shift_log: the getters read it from any thread
  // per channel: (first call, shift) of every call with a retune or reset in front of it, call order; empty until
  // the first edit (enable_retune or reset_channels sizes it)
  std::vector<std::vector<std::pair<uint32_t, int>>> shift_log;
  // per channel: the calls of shift_log with a retune in front of them (the others: resets and imports), call order
  std::vector<std::vector<uint32_t>> retune_log;
  std::vector<uint32_t> gdec_epoch;    // per channel: the edit whose reset the group decoder has seen
  struct Edit
  {
    unsigned ch;
    int shift;
    bool reset; // fmd_batch_reset_channels (shift unused); else a retune to `shift`
    int imp = -1; // >= 0: an import (fmd_batch_import_channels), entry of `imports`; the slot takes `shift`
  };
  std::vector<Edit> edits;             // pending, in the order they were made (local channel numbers)
  bool edits_pending = false;          // caller-facing batch: edits wait in `edits` here or in a sub-batch
  fmd::RestartTable restart_tab{};
  int restart_group[fmd::kRestartMaxRegions] = {}; // region of restart_regions each table entry belongs to
  int restart_skip = -1;               // fmd_batch_debug_set "restart_skip" (mutation test): a region left out
  unsigned restart_rows_cap = 0;       // distinct tuner rows one restart can carry
  HostBuf<int2> h_edits;               // [NSLOT][2 C] page-locked staging of the edit lists (restarts, resets)
  HostBuf<float2> h_rows;              // [NSLOT][restart_rows_cap * table_size] ... and of the new tuner rows
  DevBuf<int2> d_edits;
  DevBuf<float2> d_rows;
  Event edit_ev[NSLOT];                // behind the copy out of a staging slot
  Event edit_done;                     // behind the restart (the twin's next call waits where streams differ)
  unsigned restart_seq = 0;
  /* Resetting single channels (fmd_batch_reset_channels): the ring phase of a channel's RDS
   * low-pass and matched filter is the batch's (rds_lpf_g, mf_g) minus its origin -- org[c] and org[CP + c], the
   * batch phases when it was last reset, 0 for a channel that never was.  Until a batch's first reset every origin
   * is 0 and the ring filters run without them (origins_live); fmd_batch_reset returns to that. */
  DevBuf<unsigned> org;                // [2][CP]
  bool origins_live = false;
  int dbg_reset_keep_phase = 0;        // fmd_batch_debug_reset_keep_ring_phase (test aid): origins stay 0

  /* The capture map (fmd_batch_set_capture_map / fmd_batch_switch_captures).  Every batch
   * knows the input rows a call takes (n_cap, 0: no map, the cpc rule).  A batch with buffers of its own holds its
   * channels' captures as its next call reads them (cmap, local channel numbers, global capture rows) and the walk
   * table its IF stage reads: (channel, capture) per block row, the channels sorted by capture where capture_walk
   * is on.  A changed map goes to d_walk in front of the next call's IF stage, on that stage's stream, out of a
   * page-locked staging slot per call index mod NSLOT: the IF stages of consecutive calls run in order on that
   * stream (each reads the IF history the previous one wrote), so calls submitted earlier read the old table. */
  unsigned n_cap = 0;
  bool map_on = false, map_dirty = false;
  int capture_walk = 1;                // fmd_batch_debug_capture_walk (development switch)
  std::vector<unsigned> cmap;          // [C]
  DevBuf<uint2> d_walk;                // [C]
  HostBuf<uint2> h_walk;               // [NSLOT][C]
  Event walk_ev[NSLOT];                // behind the copy out of a staging slot

  /* Saving, loading and moving channel state (fmd_batch_save_state and its kin).  A batch
   * with buffers of its own holds the table of its carried regions (state_tab, built on first use: the restart's
   * regions, the status record and the clip counter), the bytes a channel takes in a payload, and the imports its
   * next call applies: each staged in a page-locked slot (list entries, tuner rows, packed payload) that one copy
   * takes to the device slot of the same number in front of k_channel_import.  The caller-facing batch holds the
   * group decoders that come with imported channels until a group of their first call arrives. */
  fmd::StateTable state_tab{};
  int state_group[fmd::kStateMaxRegions] = {}; // the skip index each table entry belongs to (0..10)
  size_t state_bytes = 0;              // per channel, device payload
  int state_skip = -1;                 // fmd_batch_debug_state_skip (mutation test): a region loads / imports leave out
  struct PendingImport
  {
    int slot = 0;
    unsigned n_cols = 0, n_rows = 0;   // channels of the blob, distinct tuner rows
    size_t rows_at = 0, payload_at = 0, bytes = 0; // layout of the staging slot
    bool origins_live = false;
    std::vector<fmd::StateEdit> list;  // this batch's channels of the import, sorted by channel
  };
  std::vector<PendingImport> imports;
  HostBuf<char> h_imp[NSLOT];
  DevBuf<char> d_imp[NSLOT];
  Event imp_ev[NSLOT];                 // behind the copy out of a staging slot
  unsigned imp_seq = 0;
  struct GdecImport
  {
    uint32_t k = 0;                    // first call of the imported decoder
    std::unique_ptr<fmd::GroupDecoder> g; // null: the record had none yet
  };
  std::map<unsigned, std::vector<GdecImport>> gdec_imports; // caller-facing batch, per channel, call order
  // baseband samples the batch-wide oscillator sequence still lacks as history (a load from a batch that kept none:
  // until then the serial stage writes mixed rows)
  unsigned osc_warm = 0;

  // Everything else frees itself; the sub-batches and the twin run on this batch's streams: they go first.
  ~fmd_batch()
  {
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    subs.clear();
    twin.reset();
    if (owns_streams)
      for (hipStream_t st : {s_fir, s_ser, s_post, s_rds, s_lpf})
        if (st)
          (void)hipStreamDestroy(st);
  }
};

namespace
{

constexpr unsigned kMaxProfCalls = 512;
// channels of one batch with buffers of its own: 64 CUs' worth of the whole-CU serial stage (128 channels per CU), the
// size the pipeline is balanced for.  (Measured, round 6: ONE batch of 8320 channels = 65 CUs still runs at the
// 8192-channel rate, 8448 / 8704 / 9216 lose 10-13 % -- profiles/r6_f_*: no headroom above it worth a special case.)
constexpr unsigned kSubBatchChannels = 8192;

inline bool is_shell(const fmd_batch* b)
{
  return !b->subs.empty();
}

/* A caller-facing batch and the batches with buffers of their own behind it: a shell's sub-batches with their first
 * channels, or the plain batch itself.  THE walk over "every part": whatever is done per batch with buffers goes
 * through it (what recurses through a sub-batch as a whole batch -- waits, resets, error words -- does not). */
struct Part
{
  fmd_batch* x;
  unsigned ch0;
};
std::vector<Part> parts(fmd_batch* b)
{
  std::vector<Part> v;
  for (size_t k = 0; k < b->subs.size(); k++)
    v.push_back(Part{b->subs[k].get(), b->sub_ch0[k]});
  if (v.empty())
    v.push_back(Part{b, 0u});
  return v;
}
inline fmd_batch* first_part(fmd_batch* b)
{
  return is_shell(b) ? b->subs[0].get() : b;
}

/* a batch-wide setting that every sub-batch mirrors: the batch's own copy and theirs */
template <typename T, typename V>
void set_all(fmd_batch* b, T fmd_batch::*member, const V& value)
{
  b->*member = value;
  for (auto& sb : b->subs)
    sb.get()->*member = value;
}

/* whether the batch's next call writes any audio row (a selection of no rows: the audio pointer may be null) */
inline bool audio_rows_due(const fmd_batch* b)
{
  return !(b->sel[FMT_PCM].on && b->sel[FMT_PCM].n_total == 0);
}

/* The baseband lengths a call with channel IQ rows as input may have (fmd_batch_baseband_limits): those an IQ call
 * can produce -- from the smallest call's (fmd_batch_min_samples / D, in every decimator phase) to the largest
 * block's, D samples apart each. */
inline unsigned baseband_min(const fmd_batch* b)
{
  return b->min_samples / b->des.D;
}
inline unsigned baseband_max(const fmd_batch* b)
{
  return b->Mmax - 1; // (Mmax: one more than the decimator's outputs of the largest block, fmd_batch_create)
}

/* the sub-batch that owns a channel, and the channel's index there (a plain batch: itself) */
inline fmd_batch* owner_of(fmd_batch* b, unsigned channel, unsigned* local)
{
  if (!is_shell(b))
  {
    *local = channel;
    return b;
  }
  // (sub_ch0 ends with C: the last first channel that is not above `channel`)
  const size_t s = size_t(std::upper_bound(b->sub_ch0.begin(), b->sub_ch0.end() - 1, channel) - b->sub_ch0.begin()) - 1;
  *local = channel - b->sub_ch0[s];
  return b->subs[s].get();
}

int upload(void* dst, const void* src, size_t bytes)
{
  return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}

void bind_state(fmd_batch* b)
{
  b->st.f = b->fstate.p;
  b->st.i = b->istate.p;
  b->st.r_data = b->r_data.p;
  b->st.CP = b->CP;
  void* derr = nullptr;
  if (b->h_err.p && hipHostGetDevicePointer(&derr, b->h_err.p, 0) == hipSuccess)
    b->st.err = static_cast<unsigned*>(derr);
  void* dhs = nullptr;
  if (b->h_status.p && hipHostGetDevicePointer(&dhs, b->h_status.p, 0) == hipSuccess)
    b->st.hs = static_cast<unsigned*>(dhs);
  b->st.ds = b->d_status.p;
  // bound of the serial stage's LDS hand-off waits (~0.1 s; fmd_batch_debug_set_spin_limit)
  b->st.spin_limit = b->spin_limit;
}

/* The host's own updates of the status snapshot (initial values, Reset): same protocol as the
 * kernel's (fmd::HostStatusWord), with tags no call index ever has.  Only called while no call is in
 * flight. */
void host_status_update(fmd_batch* b, const std::function<void(unsigned* rec, size_t stride)>& edit)
{
  const size_t CP = b->CP;
  const unsigned tag = 0x80000000u | ++b->host_seq;
  for (unsigned c = 0; c < b->C; c++)
  {
    unsigned* h = b->h_status.p + c;
    __atomic_store_n(&h[fmd::HS_SEQ_BEGIN * CP], tag, __ATOMIC_RELEASE);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    edit(h, CP);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    __atomic_store_n(&h[fmd::HS_SEQ_END * CP], tag, __ATOMIC_RELEASE);
  }
}

/* One channel's snapshot, consistent (taken between two equal sequence words). */
bool host_status_read(const fmd_batch* b, unsigned channel, unsigned out[fmd::HS_WORDS])
{
  const size_t CP = b->CP;
  const unsigned* h = b->h_status.p + channel;
  for (int tries = 0; tries < 100000; tries++)
  {
    const unsigned e = __atomic_load_n(&h[fmd::HS_SEQ_END * CP], __ATOMIC_ACQUIRE);
    for (int w = fmd::HS_SEQ_BEGIN + 1; w < fmd::HS_SEQ_END; w++)
      out[w] = __atomic_load_n(&h[size_t(w) * CP], __ATOMIC_RELAXED);
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    const unsigned g = __atomic_load_n(&h[fmd::HS_SEQ_BEGIN * CP], __ATOMIC_ACQUIRE);
    if (e == g)
    {
      out[fmd::HS_SEQ_BEGIN] = out[fmd::HS_SEQ_END] = e;
      return true;
    }
  }
  return false; // a writer that never finishes: only a hung device
}

/* A step that cannot report through its return value (stream bookkeeping inside a launch helper)
 * failed: the batch refuses further calls (see check_device_errors). */
void mark_failed(fmd_batch* b, const char* what)
{
  if (!b->failed)
  {
    b->failed = true;
    b->fail_msg = what;
  }
}

/* Turns the device-side error word, and an earlier broken-off call, into an error code. */
int check_device_errors(fmd_batch* b)
{
  if (!b->subs.empty())
  { // a shell: its sub-batches' words; one that failed fails the whole batch
    for (auto& sb : b->subs)
      if (check_device_errors(sb.get()) != FMD_OK && !b->failed)
      {
        b->failed = true;
        b->fail_msg = sb->fail_msg;
      }
    return b->failed ? fail(FMD_ERR_DEVICE, b->fail_msg) : FMD_OK;
  }
  const unsigned e = b->h_err.p ? __atomic_load_n(&b->h_err.p[0], __ATOMIC_ACQUIRE) : 0u;
  if (e && !b->failed)
  {
    b->failed = true;
    b->fail_msg = "device-side error:";
    if (e & fmd::DEVERR_SERIAL_HANDSHAKE)
      b->fail_msg += " serial stage hand-off timed out (results of that call are invalid)";
  }
  if (b->failed)
    return fail(FMD_ERR_DEVICE, b->fail_msg);
  return FMD_OK;
}

/* RDS groups that did not fit a queue or the caller's record buffer are lost, nothing else: audio and
 * channel state are intact and the batch stays usable.  Reported once (FMD_WARN_RDS_LOST), then
 * cleared (atomically: a kernel setting the flag again at that moment is seen by the next query). */
int take_lost_groups(fmd_batch* b)
{
  if (!b->subs.empty())
  {
    int rc = FMD_OK;
    for (auto& sb : b->subs)
      if (take_lost_groups(sb.get()) != FMD_OK)
        rc = FMD_WARN_RDS_LOST;
    return rc;
  }
  // one exchange: a kernel that ORs the flag in between a load and a store would have its loss wiped
  if (!b->h_err.p || !__atomic_exchange_n(&b->h_err.p[1], 0u, __ATOMIC_ACQ_REL))
    return FMD_OK;
  g_err = "RDS groups were lost: a call's group queue or the export buffer was full (drain every call's "
          "groups with fmd_batch_collect_rds / fmd_batch_export_rds_device, with cap >= the groups queued)";
  return FMD_WARN_RDS_LOST;
}

/* state a freshly constructed cFmDecoder has (ctor values that are not zero) */
int init_signal_state(fmd_batch* b)
{
  const size_t CP = b->CP;
  std::vector<float> v(CP);
  std::fill(v.begin(), v.end(), b->des.p_freq0); // cPilotPhaseLock: m_freq = freq*2pi (:131)
  if (upload(b->st.F(fmd::F_P_FREQ), v.data(), CP * sizeof(float)))
    return -1;
  std::fill(v.begin(), v.end(), 1.0f); // CRDSDownConvert: m_Osc1 = (1, 0) (DownConvert.cpp:284)
  if (upload(b->st.F(fmd::F_OSC_RE), v.data(), CP * sizeof(float)))
    return -1;
  return 0;
}

/* What cFmDecoder::Reset (FmDecode.cpp:326-338) + cRDSRxSignalProcessor::Reset (RDSProcess.cpp:92-118) clear on
 * the device, per channel: the demod / RDS recurrences, the T-1 history rows of the RDS low-pass (both parities of
 * rdsraw) and of the matched filter (rpll), and the status words of the meters Reset clears.  Tuner index,
 * FIR / resampler histories, pilot PLL, half-band histories, oscillator, de-emphasis, notch, audio LPF and the
 * block-sync shift register stay, like the reference.  Every region is rows x CP elements, time-major.  ONE list:
 * do_reset zeroes it for the whole batch, k_channel_reset for the channels fmd_batch_reset_channels lists; the
 * ring phases that go with it are rds_lpf_g / mf_g (whole batch) and the origins (single channels). */
std::vector<fmd::ResetRegion> reset_regions(const fmd_batch* b)
{
  using namespace fmd;
  std::vector<ResetRegion> v;
  auto add = [&](void* p, size_t rows, unsigned esz) {
    if (p && rows)
      v.push_back(ResetRegion{p, unsigned(rows), esz});
  };
  const ChannelState& s = b->st;
  for (int slot : {F_IF_LEVEL, F_BB_MEAN, F_BB_LEVEL, F_DC_OFF, F_NCO_INCR, F_NCO_PHASE, F_R_PHASE, F_R_FREQ, F_R_W1,
                   F_R_W2, F_R_LAST_SYNC, F_R_LAST_SLOPE, F_R_LAST_DATA})
    add(s.F(slot), 1, 4);
  for (int slot : {I_STEREO, I_STEREO_Q0, I_STEREO_Q1, I_STEREO_Q2, I_STEREO_Q3, I_R_LAST_BIT, I_R_BITPOS, I_R_BLOCK,
                   I_R_STATE, I_R_BOFF})
    add(s.I(slot), 1, 4);
  for (int q = 0; q < 2; q++)
    add(b->rdsraw[q].p, b->des.rds_lpf_taps.size() - 1, 8);
  add(b->rpll.p, b->des.rds_mf_taps.size() - 1, 4);
  // the getters' snapshot follows: the meters Reset clears read zero, pilot level and the receiver's audio
  // meter stay (every call rewrites these words before its status record copies them)
  if (b->d_status.p)
    for (int w : {HS_IF_LEVEL, HS_BB_MEAN, HS_BB_LEVEL, HS_STEREO, HS_R_STATE})
      add(b->d_status.p + size_t(w) * b->CP, 1, 4);
  return v;
}

template <class IN>
int launch_if_stage(fmd_batch* b, const void* d_iq, size_t iq_channel_stride, unsigned N, unsigned pos,
                    unsigned M, int q, hipStream_t sF, const std::function<void(int)>& mark,
                    hipEvent_t ev_start, hipEvent_t ev_stop);

/* the whole batch: reset_regions, the ring phases, the per-channel ring origins, the group decoders */
int do_reset(fmd_batch* b)
{
  if (b->twin && do_reset(b->twin.get())) // the silent twin receives every whole-batch reset too
    return -1;
  if (!b->subs.empty())
  {
    for (auto& sb : b->subs)
      if (do_reset(sb.get()))
        return -1;
    for (auto& g : b->gdec)
      if (g)
        g->reset();
    b->failed = false;
    b->fail_msg.clear();
    return 0;
  }
  for (const fmd::ResetRegion& r : reset_regions(b))
    if (hipMemset(r.dst, 0, size_t(r.rows) * b->CP * r.esz) != hipSuccess)
      return -1;
  if (b->org.p && hipMemset(b->org.p, 0, b->org.n * sizeof(unsigned)) != hipSuccess)
    return -1;
  b->origins_live = false; // every channel in the batch's phase again: the ring filters without origins
  b->rds_lpf_g = 0;
  b->mf_g = 0;
  for (auto& g : b->gdec)
    if (g)
      g->reset();
  if (b->h_err.p)
  {
    __atomic_store_n(&b->h_err.p[0], 0u, __ATOMIC_RELEASE);
    __atomic_store_n(&b->h_err.p[1], 0u, __ATOMIC_RELEASE);
  }
  b->failed = false;
  b->fail_msg.clear();
  // the host's copy of the snapshot: the words reset_regions zeroes in the device record
  if (b->h_status.p)
    host_status_update(b, [](unsigned* h, size_t CP) {
      for (int w : {fmd::HS_IF_LEVEL, fmd::HS_BB_MEAN, fmd::HS_BB_LEVEL, fmd::HS_STEREO, fmd::HS_R_STATE})
        __atomic_store_n(&h[size_t(w) * CP], 0u, __ATOMIC_RELAXED);
    });
  return 0;
}

/* HIP multiplexes streams onto a few hardware queues, and two of this library's chains on one
 * queue block each other (the FIR of the next call would queue behind the previous call's post
 * chain: measured -13 % when just one unrelated stream created earlier shifted the assignment).
 * So the internal streams are picked by measurement: candidates are created until `n` of them run
 * a no-op kernel at once while all already chosen ones are kept busy by a spinning wave. */
int pick_independent_streams(int n, const int* priority, hipStream_t* out, int* n_sharing)
{ // *n_sharing: how many of the n streams had to be taken although the probe found them behind another one
  std::vector<hipStream_t> rejected;
  int have = 0;
  for (int attempt = 0; attempt < 24 && have < n; attempt++)
  {
    hipStream_t cand = nullptr;
    if (hipStreamCreateWithPriority(&cand, hipStreamNonBlocking, priority[have]) != hipSuccess)
      break;
    bool independent = true;
    {
      const long long spin = 1200000; // ~0.5 ms
      for (int i = 0; i < have; i++)
        hipLaunchKernelGGL(fmd::k_probe_spin, dim3(1), dim3(64), 0, out[i], spin, nullptr);
      // the default stream too: it is the caller's stream more often than not
      hipLaunchKernelGGL(fmd::k_probe_spin, dim3(1), dim3(64), 0, nullptr, spin, nullptr);
      const auto t0 = std::chrono::steady_clock::now();
      hipLaunchKernelGGL(fmd::k_probe_nop, dim3(1), dim3(64), 0, cand, nullptr);
      (void)hipStreamSynchronize(cand);
      const double us =
          std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
      independent = us < 250.0; // behind a spinning wave it would take ~500 us
      for (int i = 0; i < have; i++)
        (void)hipStreamSynchronize(out[i]);
      (void)hipStreamSynchronize(nullptr);
    }
    if (independent)
      out[have++] = cand;
    else
      rejected.push_back(cand);
  }
  // whatever is still missing (no independent queue left): take the rejected ones, it still works
  *n_sharing = 0;
  while (have < n && !rejected.empty())
  {
    out[have++] = rejected.back();
    rejected.pop_back();
    ++*n_sharing;
  }
  for (hipStream_t s : rejected)
    (void)hipStreamDestroy(s);
  return have == n ? 0 : -1;
}

/* The steps of k_halfband_chain for a call of n_in inputs cut into S stretches of the last stage's
 * outputs (see the kernel): per step how far each stage runs -- at most 16 / 8 / 4 outputs, no further
 * than its input ring has rows for, and never onto a ring row the next stage still needs. */
fmd_batch::HbfPlan* hbf_plan(fmd_batch* b, unsigned n_in, unsigned S)
{
  for (auto& pl : b->hbf_plans)
    if (pl->n_in == n_in && pl->S == S)
      return pl.get();
  const fmd::Design& d = b->des;
  const int L1H = d.hb[1].len - 1, L2H = d.hb[2].len - 1, RING = fmd::HBF_RING;
  const int n0 = int(n_in + 1) / 2, n1 = (n0 + 1) / 2, n2 = (n1 + 1) / 2;
  std::vector<fmd::HbStep> steps;
  std::vector<int> first;
  const int per = (n2 + int(S) - 1) / int(S);
  fmd::HbTails tails{};
  tails.tail1 = b->hbf_tail1.p;
  tails.tail2 = b->hbf_tail2.p;
  tails.first1 = n0 - L1H;
  tails.first2 = n1 - L2H;
  for (int a = 0; a < n2; a += per)
  {
    first.push_back(int(steps.size()));
    const size_t f = steps.size();
    const int e = std::min(n2, a + per);
    // what the stretch's outputs need of stages 1 and 0; the call's last stretch also computes the outputs
    // behind that (they are part of the delay lines the next call starts from)
    const bool last = e == n2;
    const int need1 = last ? n1 : 2 * (e - 1) + 1, need0 = last ? n0 : 2 * (need1 - 1) + 1;
    int d2 = a, d1 = std::max(0, 2 * a - L2H), d0 = std::max(0, 2 * d1 - L1H);
    auto push = [&](int an, int bn, int cn) {
      unsigned n = unsigned(an) | unsigned(bn) << 5 | unsigned(cn) << 9;
      if (an > 0 && d0 + an > tails.first1)
        n |= fmd::HBF_TAIL0;
      if (bn > 0 && d1 + bn > tails.first2)
        n |= fmd::HBF_TAIL1;
      steps.push_back(fmd::HbStep{d0, d1, d2, n});
    };
    while (d2 < e || d1 < need1 || d0 < need0)
    {
      const int a_hi = std::max(d0, std::min({d0 + 16, need0, 2 * d1 - L1H + RING}));
      const int b_hi = std::max(d1, std::min({d1 + 8, need1, a_hi > 0 ? (a_hi - 1) / 2 + 1 : 0, 2 * d2 - L2H + RING}));
      const int c_hi = std::max(d2, std::min({d2 + 4, e, b_hi > 0 ? (b_hi - 1) / 2 + 1 : 0}));
      if (a_hi == d0 && b_hi == d1 && c_hi == d2)
        return nullptr; // cannot happen: a stage can always move
      push(a_hi - d0, b_hi - d1, c_hi - d2);
      d0 = a_hi;
      d1 = b_hi;
      d2 = c_hi;
    }
    while ((steps.size() - f) % fmd::HBF_NSET) // the kernel takes a stretch's steps four at a time
      push(0, 0, 0);
    // what the kernel finds in a record instead of fetching or carrying it (HbStep::n): the rows to fetch during
    // the step, the stretch's end, the way to the stretch's copy of `tails` (behind its last step)
    const size_t g = steps.size();
    for (size_t i = f; i < g; i++)
    {
      const int far = steps[std::min(i + size_t(fmd::HBF_NSET - 1), g - 1)].a_lo - steps[i].a_lo;
      if (far < 0 || far > 63 || g - i > 1023)
        return nullptr; // cannot happen: three steps of at most 16 outputs; a call has a few hundred steps
      steps[i].n |= unsigned(far) << fmd::HBF_FAR_SHIFT;
      if (steps[i].n & (fmd::HBF_TAIL0 | fmd::HBF_TAIL1))
        steps[i].n |= unsigned(g - i) << fmd::HBF_TAILS_SHIFT;
    }
    steps[g - 1].n |= fmd::HBF_LAST;
    fmd::HbStep hdr[2];
    static_assert(sizeof(hdr) == sizeof(tails), "HbTails in the place of two records");
    std::memcpy(hdr, &tails, sizeof(tails));
    steps.push_back(hdr[0]);
    steps.push_back(hdr[1]);
  }
  first.push_back(int(steps.size()));
  std::unique_ptr<fmd_batch::HbfPlan> pl(new fmd_batch::HbfPlan);
  pl->n_in = n_in;
  pl->S = unsigned(first.size() - 1);
  if (pl->steps.alloc(steps.size()) || pl->seg_first.alloc(first.size()) ||
      upload(pl->steps.p, steps.data(), steps.size() * sizeof(fmd::HbStep)) ||
      upload(pl->seg_first.p, first.data(), first.size() * sizeof(int)))
    return nullptr;
  if (b->hbf_plans.size() >= 16) // call sizes keep changing: forget the oldest list
  {
    (void)hipDeviceSynchronize();
    b->hbf_plans.erase(b->hbf_plans.begin());
  }
  b->hbf_plans.push_back(std::move(pl));
  return b->hbf_plans.back().get();
}

/* k_resample_ring's geometry for one of its forms (outputs per wave x waves): does a step's window
 * (+ alignment, + the even-count batch) fit 39 ring batches of 4 KB, and a step's new rows the
 * registers that carry them?  Leaves rsr_R = 0 when not. */
bool rsr_configure(fmd_batch* b, int form)
{
  // 2 x 8 first: two waves per SIMD cover each other's waits (0.30 ms alone at 8192 channels against 0.36
  // for 4 x 4; 2 x 4, half the outputs per step, is what longer windows still fit: 0.87 ms)
  static const int forms[3][2] = {{2, 8}, {4, 4}, {2, 4}};
  const fmd::Design& d = b->des;
  const int R = forms[form][0], NW = forms[form][1];
  const double step = double(d.rs_step);
  const unsigned per_step = unsigned(NW * R);
  const unsigned span = d.rs_order + 1u + unsigned(std::ceil((per_step - 1) * step)) + 1u;
  const unsigned nbr = (span - 1u + 7u) / 8u + 2u;
  const unsigned new_rows = unsigned(std::ceil(per_step * step)) + 8u;
  b->rsr_R = 0;
  if (nbr > 39u || new_rows > unsigned(fmd::RSR_ROWS))
    return false;
  b->rsr_R = R;
  b->rsr_NW = NW;
  b->rsr_nbr = nbr;
  b->rsr_rb = int((d.rs_order + 7u) / 8u * 8u + 8u);
  const unsigned gspan = d.rs_order + 1u + unsigned(std::ceil((R - 1) * step)) + 1u;
  b->rsr_nbm = (gspan - 1u + 7u) / 8u + 2u + 1u; // + 1: the walk's dummy last load
  return true;
}

} // namespace

extern "C" {

const char* fmd_last_error(void)
{
  return g_err.c_str();
}

const char* fmd_version(void)
{
  return "fmd-hip 0.1 (gfx950)";
}

const char* fmd_stage_name(unsigned idx)
{
  return idx < ST_COUNT ? kStageNames[idx] : "";
}

} // extern "C"

namespace
{

/* The internal streams of a batch: the FIR feeds the pipeline and is the bandwidth-bound kernel -- dispatch it
 * first; the post chain has slack every call and goes last. */
int create_streams(fmd_batch* b)
{
  int lo = 0, hi = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi)); // lo = least, hi = greatest priority
  // (the two heavy chains side by side on a fifth stream: measured slower in rounds 1-3, removed.)  The
  // fifth stream carries the post chain's two low-pass filters or the light part's audio half: see the stream
  // layouts in front of submit_overlapped
  const int nstreams = 5;
  // (the light chain's stream at the high priority too: measured twice, no difference; the heavy part's,
  // which since round 4 is on the loop that closes the period: 279 100 against 279 200 MS/s; with the
  // low-pass filters' as well: -1.6 %)
  const int prio[5] = {hi, hi, lo, lo, lo};
  hipStream_t st4[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  if (pick_independent_streams(nstreams, prio, st4, &b->streams_sharing) != 0)
    return fail(FMD_ERR_DEVICE, "could not create the internal streams");
  b->s_fir = st4[0];
  b->s_ser = st4[1];
  b->s_post = st4[2];
  b->s_rds = st4[3];
  b->s_lpf = st4[4];
  return FMD_OK;
}

/* One batch with buffers and state of its own: what fmd_batch_create returns up to kSubBatchChannels channels, and
 * every sub-batch of a larger one (shell != null: on the shell's streams). */
int create_one(const fmd_params* params, unsigned n_channels, const int* tuning_shifts, int device,
               const fmd_callbacks* cb, void* user, fmd_batch* shell, fmd_batch** out)
{
  std::unique_ptr<fmd_batch> b(new fmd_batch);
  b->device = device;
  b->cparams = *params;
  b->params.sample_rate_if = params->sample_rate_if;
  b->params.tuning_offset = params->tuning_offset;
  b->params.sample_rate_pcm = params->sample_rate_pcm;
  b->params.bandwidth_pcm = params->bandwidth_pcm;
  b->params.downsample = params->downsample;
  b->params.us_version = params->us_version != 0;
  b->params.table_size = params->table_size;
  b->params.if_filter_order = params->if_filter_order;
  if (params->fir_reduction != FMD_FIR_SEQUENTIAL && params->fir_reduction != FMD_FIR_SHUFFLE_PARITY_WAIVED &&
      params->fir_reduction != FMD_FIR_FMA_PARITY_WAIVED)
    return fail(FMD_ERR_ARG, "fmd_batch_create: fir_reduction must be 0 (sequential, the parity mode), "
                             "FMD_FIR_FMA_PARITY_WAIVED (fused multiply-add in the reference's tap order) or "
                             "FMD_FIR_SHUFFLE_PARITY_WAIVED (shuffle-reduced: 1.2e-5 RMS from the reference, "
                             "outside the 1e-5 contract)");
  b->params.fir_reduction = params->fir_reduction == FMD_FIR_SHUFFLE_PARITY_WAIVED ? 1
                            : params->fir_reduction == FMD_FIR_FMA_PARITY_WAIVED   ? 2
                                                                                   : 0;
  try
  {
    b->des = fmd::make_design(b->params);
  }
  catch (const std::exception& e)
  {
    return fail(FMD_ERR_ARG, e.what());
  }
  const fmd::Design& d = b->des;
  { // Smallest call.  Short blocks are decoded like the reference decodes them (a half-band stage
    // below L inputs passes its input on unfiltered, below 2 (L - 1) it refills its delay line from
    // outputs, a block shorter than a filter keeps part of the old history: stage_decimator_stages);
    // what is refused are only blocks so short that a stage would be left with NO sample -- there the
    // reference divides by zero in its level meters (FmDecode.cpp:522-539, RadioReceiver.cpp:584-598)
    // -- and blocks that give the unrolled 11-tap class fewer inputs than it reads unconditionally.
    // The bound holds in every phase of the decimator: baseband samples M >= N / D rounded down.
    unsigned mmin = 5; // an audio frame falls into every block of >= ceil(step) + 1 baseband samples
    while (double(mmin) < double(d.rs_step) + 1.0)
      mmin++;
    for (;; mmin++)
    {
      unsigned n = mmin;
      bool ok = true;
      for (const auto& h : d.hb)
      {
        if (h.cic)
        { // (an even number of inputs: stage_decimator_stages)
          ok = ok && n >= 2 && n % 2 == 0;
          n = n / 2;
        }
        else if (h.len == 11)
        {
          ok = ok && n >= 20;
          n = n / 2;
        }
        else
          n = n < unsigned(h.len) ? n / 2 : (n + 1) / 2;
      }
      if (ok && n >= 1)
        break;
    }
    const unsigned long long need = 1ull * mmin * d.D;
    if (need > FMD_MAX_BLOCK)
      return fail(FMD_ERR_ARG, "this geometry needs calls longer than the largest block (65536 samples)");
    b->min_samples = unsigned(need);
  }
  if (cb)
    b->cb = *cb;
  b->user = user;
  const unsigned C = n_channels;
  const unsigned CP = (C + 63u) & ~63u;
  b->C = C;
  b->CP = CP;

  // cFineTuner tables, one per channel
  b->shifts.resize(C);
  const int def_shift = fmd::tuning_shift_for(b->params);
  std::vector<float> lut(size_t(2) * d.table_size * C);
  for (unsigned c = 0; c < C; c++)
  {
    b->shifts[c] = tuning_shifts ? tuning_shifts[c] : def_shift;
    if (c > 0 && b->shifts[c] == b->shifts[c - 1])
      std::copy_n(&lut[size_t(2) * d.table_size * (c - 1)], 2 * d.table_size, &lut[size_t(2) * d.table_size * c]);
    else
    {
      auto t = fmd::make_tuner_lut(d.table_size, b->shifts[c]);
      std::copy(t.begin(), t.end(), &lut[size_t(2) * d.table_size * c]);
    }
  }

  // geometry
  b->Mmax = (FMD_MAX_BLOCK + d.D - 1) / d.D + 1;
  b->Mstride = (b->Mmax + 15u) & ~15u;
  b->Amax = unsigned(double(b->Mmax) / double(d.rs_step)) + 4;
  {
    unsigned n = b->Mmax;
    for (size_t s = 0; s < d.hb.size(); s++)
    {
      b->hb_nmax.push_back(n);
      n = (n + 1) / 2;
    }
    b->Rmax = n;
  }
  const unsigned T_lpf = unsigned(d.rds_lpf_taps.size());
  const unsigned T_mf = unsigned(d.rds_mf_taps.size());
  const unsigned T_alp = unsigned(d.lpf_taps.size());

  /* The serial stage addresses its input rows (demod) and its two output row buffers with 32-bit
   * byte offsets per lane (fmd_kernels.hip.h, k_demod_serial): a batch stays below 4 GB in each.  At
   * 2.4 MS/s that is ~80 000 channels; at 400 kS/s (no decimation) 8 000. */
  if (size_t(b->Mstride) * C * sizeof(float2) + 4096 >= (size_t(1) << 32) ||
      size_t(b->Mmax) * CP * sizeof(float2) >= (size_t(1) << 32))
    return fail(FMD_ERR_ARG, "too many channels for one batch at this sample rate (4 GB per row buffer): split the batch");
  int bad = 0;
  bad |= b->lut.alloc(size_t(d.table_size) * C);
  bad |= b->hist[0].alloc(size_t(d.if_order) * C);
  bad |= b->hist[1].alloc(size_t(d.if_order) * C);
  // + DS: the serial stage loads whole chunks, also behind the last sample of the last channel
  bad |= b->demod[0].alloc(size_t(b->Mstride) * C + fmd::DS);
  bad |= b->demod[1].alloc(size_t(b->Mstride) * C + fmd::DS);
  bad |= b->if_coeff.alloc(d.if_coeff.size() + 64); // zero padding: fir_long_e1_asm's dummy load
  bad |= b->rs_coeff.alloc(d.rs_coeff.size());
  // rows of zeros in front: the resamplers' last batch reaches below the window (k_resample: RS_B rows,
  // k_resample_ring: down to the batch border below, + one batch); 8 rows behind: its top batch
  static_assert(fmd_batch::kBrFront >= 2 * fmd::RS_B, "front rows of br");
  // (HBF_SLACK: rows behind the last one that k_halfband_chain reads and never uses, here and behind mix[])
  bad |= b->br[0].alloc(size_t(fmd_batch::kBrFront + d.rs_order + b->Mmax + 8 + fmd::HBF_SLACK) * CP);
  bad |= b->br[1].alloc(size_t(fmd_batch::kBrFront + d.rs_order + b->Mmax + 8 + fmd::HBF_SLACK) * CP);
  if (d.hb.empty())
    return fail(FMD_ERR_ARG, "baseband rate too low for the RDS decimation chain");
  bad |= b->mix[0].alloc(size_t(d.hb[0].len - 1 + b->Mmax + fmd::HBF_SLACK) * CP);
  bad |= b->mix[1].alloc(size_t(d.hb[0].len - 1 + b->Mmax + fmd::HBF_SLACK) * CP);
  b->hbbuf.resize(d.hb.size() - 1);
  for (size_t s = 1; s < d.hb.size(); s++)
    bad |= b->hbbuf[s - 1].alloc(size_t(d.hb[s].len - 1 + b->hb_nmax[s]) * CP);
  if (d.hb.size() == 3)
  {
    bad |= b->hbf_tail1.alloc(size_t(d.hb[1].len - 1) * CP);
    bad |= b->hbf_tail2.alloc(size_t(d.hb[2].len - 1) * CP);
    for (auto& t : b->osc_tab)
      bad |= t.alloc(size_t(fmd_batch::kOscH) + b->Mmax + 8 + fmd::HBF_SLACK);
    b->h_osc_stride = size_t(fmd_batch::kOscH) + b->Mmax + 8;
    bad |= b->h_osc.alloc(fmd_batch::NSLOT * b->h_osc_stride);
    for (auto& e : b->osc_ev)
      bad |= e.create() != hipSuccess;
    // the batch-wide oscillator sequence is only read by k_halfband_chain, which exists for two chains
    const int h0 = (d.hb[0].len - 1) / 2, h1 = (d.hb[1].len - 1) / 2, h2 = (d.hb[2].len - 1) / 2;
    const bool chain_kind = h0 == 7 && ((h1 == 11 && h2 == 21) || (h1 == 9 && h2 == 17));
    b->osc_on = chain_kind && CP / 64 >= 64 && d.hb[0].len - 1 <= int(fmd_batch::kOscH);
  }
  // (the inputs of the two low-pass filters by call parity too, history rows in front: the decimator /
  // resampler of the next call does not wait for this call's low-pass)
  bad |= b->rdsraw[0].alloc(size_t(T_lpf - 1 + b->Rmax) * CP);
  bad |= b->rdsraw[1].alloc(size_t(T_lpf - 1 + b->Rmax) * CP);
  bad |= b->rlpf[0].alloc(size_t(b->Rmax) * CP);
  bad |= b->rlpf[1].alloc(size_t(b->Rmax) * CP);
  bad |= b->rpll.alloc(size_t(T_mf - 1 + b->Rmax) * CP);
  bad |= b->rmf.alloc(size_t(b->Rmax) * CP);
  bad |= b->tap_sync.alloc(size_t(b->Rmax) * CP);
  bad |= b->rs[0].alloc(size_t(T_alp - 1 + b->Amax) * CP);
  bad |= b->rs[1].alloc(size_t(T_alp - 1 + b->Amax) * CP);
  bad |= b->alp[0].alloc(size_t(b->Amax) * CP);
  bad |= b->alp[1].alloc(size_t(b->Amax) * CP);
  bad |= b->rds_lpf_taps.alloc(T_lpf);
  bad |= b->mf_taps2.alloc(size_t(2) * T_mf);
  bad |= b->audio_taps.alloc(2 * size_t(T_alp)); // twice in a row: k_audio_lpf_tail29 reads T taps from any a0
  b->rs_margin = fmd::rs_table_margin(d.rs_step); // zeros around every output's taps: k_resample
  b->rs_row = d.rs_order + 1 + 2 * b->rs_margin;
  bad |= b->ktab.alloc(size_t(b->Amax) * b->rs_row + 64);
  bad |= b->pidx.alloc(b->Amax);
  { // k_resample_ring
    hipDeviceProp_t prop{};
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
      b->n_cus = prop.multiProcessorCount;
    size_t tab_floats = 0, head_ints = 0, step_ints = 0;
    for (int form = 0; form < 3; form++)
      if (rsr_configure(b.get(), form))
      {
        const size_t per_step = size_t(b->rsr_NW) * b->rsr_R;
        const size_t nsteps = (size_t(b->Amax) + per_step - 1) / per_step;
        tab_floats = std::max(tab_floats, nsteps * b->rsr_NW * b->rsr_nbm * 8 * b->rsr_R + 256);
        head_ints = std::max(head_ints, nsteps * b->rsr_NW * fmd::RSR_HEAD);
        step_ints = std::max(step_ints, nsteps * 2);
      }
    for (int form = 0; form < 3 && !rsr_configure(b.get(), form); form++) // the first form that fits stays
      ;
    if (tab_floats)
    {
      bad |= b->rsr_tab.alloc(tab_floats);
      bad |= b->rsr_head.alloc(head_ints);
      bad |= b->rsr_steps.alloc(step_ints);
      const void* fns[] = {reinterpret_cast<const void*>(&fmd::k_resample_ring<4, 4>),
                           reinterpret_cast<const void*>(&fmd::k_resample_ring<2, 8>),
                           reinterpret_cast<const void*>(&fmd::k_resample_ring<2, 8, true>),
                           reinterpret_cast<const void*>(&fmd::k_resample_ring<2, 4>)};
      for (const void* f : fns)
        (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64);
    }
  }
  if (b->params.fir_reduction == 2)
  { // the fused multiply-add form of the resamplers is the ring kernel's, two outputs x eight waves: every call takes it
    if (b->rsr_R != 2 || b->rsr_NW != 8)
      return fail(FMD_ERR_ARG, "FMD_FIR_FMA_PARITY_WAIVED: the fused multiply-add form exists for the reference "
                               "geometry only (this resampler window does not fit the 2 x 8 ring form)");
    b->rsr_mode = 1;
  }
  bad |= b->sctab.alloc(d.sincos_tab.size());
  bad |= b->sctab256.alloc(d.sincos_tab256.size());
  bad |= b->fstate.alloc(size_t(fmd::F_SLOTS) * CP);
  bad |= b->pcm_clip.alloc(CP);
  bad |= b->istate.alloc(size_t(fmd::I_SLOTS) * CP);
  bad |= b->r_data.alloc(size_t(4) * CP);
  bad |= b->groups.alloc_queues(std::max(4096u, 8u * C));
  bad |= b->groups.alloc_counts();
  bad |= b->export_cursor.alloc(fmd_batch::kExportCursors);
  if (bad)
    return fail(FMD_ERR_DEVICE, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()));

  bad |= upload(b->lut.p, lut.data(), lut.size() * sizeof(float));
  bad |= upload(b->if_coeff.p, d.if_coeff.data(), d.if_coeff.size() * sizeof(float));
  bad |= upload(b->rs_coeff.p, d.rs_coeff.data(), d.rs_coeff.size() * sizeof(float));
  bad |= upload(b->rds_lpf_taps.p, d.rds_lpf_taps.data(), T_lpf * sizeof(float));
  bad |= upload(b->audio_taps.p, d.lpf_taps.data(), T_alp * sizeof(float));
  bad |= upload(b->audio_taps.p + T_alp, d.lpf_taps.data(), T_alp * sizeof(float));
  bad |= upload(b->sctab.p, d.sincos_tab.data(), d.sincos_tab.size() * sizeof(double));
  bad |= upload(b->sctab256.p, d.sincos_tab256.data(), d.sincos_tab256.size() * sizeof(double));
  bad |= upload(b->mf_taps2.p, d.rds_mf_taps.data(), T_mf * sizeof(float));
  for (const auto& h : d.hb)
  {
    fmd::HbCoef hc{};
    for (int i = 0; i < h.len; i++)
      hc.c[i] = h.coef[size_t(i)];
    for (int j = 0; 2 * j < h.len && j < 28; j++)
      hc.e[j] = hc.c[2 * j];
    b->hbcoef.push_back(hc);
  }
  if (d.hb.size() == 3)
  { // per stage the even taps and then the centre tap, one stage behind the other (HbChainTaps)
    float* t = &b->hb_taps.p[0].x;
    int k = 0;
    for (const auto& h : d.hb)
    {
      const int half = (h.len - 1) / 2;
      for (int j = 0; j <= half && k < fmd::HBF_TAPS; j++)
        t[k++] = h.coef[size_t(2 * j)];
      if (k < fmd::HBF_TAPS)
        t[k++] = h.coef[size_t(half)];
    }
  }
  // coherent (fine-grained) host memory: the kernels' system-scope writes are visible to the host
  // without a synchronisation, whatever HIP_HOST_COHERENT says
  if (b->h_err.alloc(2, hipHostMallocMapped | hipHostMallocCoherent))
    return fail(FMD_ERR_DEVICE, "host-mapped error word allocation failed");
  // (zero-filled: a fresh decoder, all meters zero)
  if (b->h_status.alloc(size_t(fmd::HS_WORDS) * CP, hipHostMallocMapped | hipHostMallocCoherent))
    return fail(FMD_ERR_DEVICE, "host-mapped status snapshot allocation failed");
  if (b->d_status.alloc(size_t(fmd::HS_WORDS) * CP))
    return fail(FMD_ERR_DEVICE, "status record allocation failed");
  // single-channel edits (fmd_batch_reset_channels, fmd_batch_retune_channels): the ring origins and the staging of
  // the edit lists, a slot per call index mod NSLOT with room for every channel's restart and reset
  if (b->org.alloc(size_t(2) * CP) || b->d_edits.alloc(size_t(fmd_batch::NSLOT) * 2 * C))
    return fail(FMD_ERR_DEVICE, "device allocation of the channel edit state failed");
  if (b->h_edits.alloc(size_t(fmd_batch::NSLOT) * 2 * C))
    return fail(FMD_ERR_DEVICE, "page-locked staging allocation failed");
  for (auto& e : b->edit_ev)
    HIPCHK(e.create());
  bind_state(b.get());
  if (!b->st.err || !b->st.hs)
    return fail(FMD_ERR_DEVICE, "host-mapped memory has no device address");
  bad |= init_signal_state(b.get());
  if (bad)
    return fail(FMD_ERR_DEVICE, "upload of constants failed");
  if (do_reset(b.get())) // the cFmDecoder ctor ends with Reset() (FmDecode.cpp:313)
    return fail(FMD_ERR_DEVICE, "state reset failed");

  b->gdec.resize(C);
  if (shell)
  {
    b->owns_streams = false;
    b->s_fir = shell->s_fir;
    b->s_ser = shell->s_ser;
    b->s_post = shell->s_post;
    b->s_rds = shell->s_rds;
    b->s_lpf = shell->s_lpf;
    b->streams_sharing = shell->streams_sharing;
  }
  else if (int rc = create_streams(b.get()))
    return rc;
  // RDS chain and audio chain behind the serial stage are independent, but side by side their kernels only
  // stretch the latency-bound serial stage (-4 % at 8192 channels), so they share one stream -- except in a batch
  // of one or two wavefronts (the single decoder of cFmDecoder: RadioReceiver.cpp:515-538), which is pure
  // latency: its RDS chain (0.35 ms of lane-serial kernels) and its audio chain (0.19 ms) run side by side,
  // 2.17 -> 1.9 ms per call of one channel ("split_post" of fmd_batch_debug_set overrides).
  b->split_post = b->CP <= 128;
  // The serial stage takes whole CUs (one role wave per SIMD; at most 64 CUs = a quarter of the chip at
  // kSubBatchChannels; +4.4 % there) where the batch is big enough for the bandwidth kernels to notice their
  // neighbours at all ("serial_exclusive" of fmd_batch_debug_set overrides).
  b->serial_exclusive = b->CP <= kSubBatchChannels && b->CP >= 1024;
  for (auto& row : b->cev)
    for (auto& e : row)
      HIPCHK(e.create());
  for (auto& e : b->ev_drained)
    HIPCHK(e.create());
  HIPCHK(hipDeviceSynchronize());
  { // can the IF stage of this geometry be launched at all (window in LDS)?  Decided here, once: a
    // process call is then never refused half-way for it
    b->if_dry_run = true;
    const std::function<void(int)> nomark = [](int) {};
    const int rc = launch_if_stage<fmd::InF32>(b.get(), nullptr, 0, FMD_MAX_BLOCK, 0, b->Mmax - 1, 0, nullptr, nomark,
                                              nullptr, nullptr);
    b->if_dry_run = false;
    if (rc != FMD_OK)
      return rc;
  }
  if (b->streams_sharing > 0 && !shell)
    // not an error: the batch works, its chains just queue behind each other where they were meant to overlap.
    // The text stays in fmd_last_error() (the call still returns FMD_OK); fmd_batch_streams_sharing_queue() has
    // the number.  HIP multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless the HOST sets the
    // variable before the runtime starts -- the library reads no environment variable itself).
    (void)fail(FMD_OK, std::to_string(b->streams_sharing) +
                           " of the batch's 5 internal streams share a hardware queue with another stream of this "
                           "process: overlapped calls will be slower than measured (host: GPU_MAX_HW_QUEUES=8 "
                           "before the HIP runtime initialises)");
  *out = b.release();
  return FMD_OK;
}

} // namespace

extern "C" {

int fmd_batch_create(const fmd_params* params, unsigned n_channels, const int* tuning_shifts,
                     int device, const fmd_callbacks* cb, void* user, fmd_batch** out)
{
  if (!params || !out || n_channels == 0)
    return fail(FMD_ERR_ARG, "fmd_batch_create: null argument or zero channels");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(FMD_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= ndev)
    return fail(FMD_ERR_ARG, "fmd_batch_create: device ordinal out of range");
  HIPCHK(hipSetDevice(device));
  // (and no more channels than keep a sub-batch's row buffers below 4 GB -- create_one; only low decimations)
  unsigned sub_cap = kSubBatchChannels;
  {
    const size_t Dd = std::max(1u, params->downsample);
    const size_t mstride = ((FMD_MAX_BLOCK + Dd - 1) / Dd + 1 + 15) & ~size_t(15);
    const size_t fit = ((size_t(1) << 32) - 8192) / (mstride * sizeof(float2)) / 128 * 128;
    sub_cap = unsigned(std::max<size_t>(128, std::min<size_t>(sub_cap, fit)));
  }
  if (n_channels <= sub_cap)
    return create_one(params, n_channels, tuning_shifts, device, cb, user, nullptr, out);

  /* A shell over sub-batches (see fmd_batch::subs): equal sizes, multiples of 128 channels (a CU's worth of
   * serial stage), so that every sub-batch call is the same load. */
  std::unique_ptr<fmd_batch> b(new fmd_batch);
  b->device = device;
  if (int rc = create_streams(b.get()))
    return rc;
  const unsigned S = (n_channels + sub_cap - 1) / sub_cap;
  const unsigned per = ((n_channels + S - 1) / S + 127u) & ~127u;
  for (unsigned ch0 = 0; ch0 < n_channels; ch0 += per)
  {
    fmd_batch* sub = nullptr;
    const unsigned n = std::min(per, n_channels - ch0);
    // (callbacks: the shell runs the group decoders, with the caller's channel numbers)
    if (int rc = create_one(params, n, tuning_shifts ? tuning_shifts + ch0 : nullptr, device, nullptr, nullptr,
                            b.get(), &sub))
      return rc;
    sub->concurrency = 2; // the sub-batch calls of one call overlap; the shell orders the caller's stream (mode 1)
    b->subs.emplace_back(sub);
    b->sub_ch0.push_back(ch0);
  }
  b->sub_ch0.push_back(n_channels);
  b->cparams = *params;
  const fmd_batch* s0 = b->subs[0].get();
  b->params = s0->params;
  b->des = s0->des;
  b->min_samples = s0->min_samples;
  b->n_cus = s0->n_cus;
  b->Mmax = s0->Mmax;
  b->Mstride = s0->Mstride;
  b->Amax = s0->Amax;
  b->C = n_channels;
  b->CP = (n_channels + 63u) & ~63u;
  for (const auto& sb : b->subs)
    b->shifts.insert(b->shifts.end(), sb->shifts.begin(), sb->shifts.end());
  if (cb)
    b->cb = *cb;
  b->user = user;
  b->gdec.resize(n_channels);
  if (b->export_cursor.alloc(fmd_batch::kExportCursors))
    return fail(FMD_ERR_DEVICE, "device allocation failed");
  HIPCHK(hipDeviceSynchronize());
  if (b->streams_sharing > 0)
    (void)fail(FMD_OK, std::to_string(b->streams_sharing) +
                           " of the batch's 5 internal streams share a hardware queue with another stream of this "
                           "process: overlapped calls will be slower than measured (host: GPU_MAX_HW_QUEUES=8 "
                           "before the HIP runtime initialises)");
  *out = b.release();
  return FMD_OK;
}

void fmd_batch_destroy(fmd_batch* b)
{
  delete b;
}

int fmd_batch_reset(fmd_batch* b)
{
  if (!b)
    return fail(FMD_ERR_ARG, "null batch");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  if (do_reset(b))
    return fail(FMD_ERR_DEVICE, "state reset failed");
  HIPCHK(hipDeviceSynchronize());
  return FMD_OK;
}

unsigned fmd_batch_channels(const fmd_batch* b)
{
  return b ? b->C : 0;
}

int fmd_batch_streams_sharing_queue(const fmd_batch* b)
{
  return b ? b->streams_sharing : -1;
}

unsigned fmd_batch_min_samples(const fmd_batch* b)
{
  return b ? b->min_samples : 0;
}

int fmd_batch_baseband_limits(const fmd_batch* b, unsigned* min, unsigned* max, unsigned* multiple)
{
  if (!b)
    return fail(FMD_ERR_ARG, "fmd_batch_baseband_limits: null batch");
  if (min)
    *min = baseband_min(b);
  if (max)
    *max = baseband_max(b);
  if (multiple)
  { // every CIC stage of the RDS decimator halves an even block (plan_call: the reference reads past an odd one)
    unsigned m = 1;
    for (const auto& h : b->des.hb)
      if (h.cic)
        m *= 2;
    *multiple = m;
  }
  return FMD_OK;
}

unsigned fmd_batch_max_mpx_samples(const fmd_batch* b, unsigned samples)
{
  // the decimator's outputs of a block, with its phase at 0 (DownConvert.cpp:112,123)
  return b ? (samples + b->des.D - 1) / b->des.D : 0;
}

double fmd_batch_mpx_rate(const fmd_batch* b)
{
  return b ? b->params.sample_rate_if / double(b->des.D) : 0.0;
}

unsigned fmd_batch_max_audio_floats(const fmd_batch* b, unsigned samples)
{
  if (!b)
    return 0;
  const unsigned M = (samples + b->des.D - 1) / b->des.D + 1;
  return 2 * (unsigned(double(M) / double(b->des.rs_step)) + 4);
}

} // extern "C"

namespace
{

/* The walk table of a batch with buffers of its own (fmd_batch::d_walk): block row i of the IF stage decodes channel
 * out[i].x from capture out[i].y.  capture_walk on: the channels sorted by capture, stable, so an ordered map walks
 * like the plain form and the channels the XCDs work on at one time read few captures (an XCD's L2 holds about one
 * capture's window, as under the cpc rule).  Off: channel order. */
void build_walk(const fmd_batch* b, uint2* out)
{
  const unsigned C = b->C;
  std::vector<unsigned> order(C);
  for (unsigned c = 0; c < C; c++)
    order[c] = c;
  if (b->capture_walk)
    std::stable_sort(order.begin(), order.end(),
                     [&](unsigned a, unsigned z) { return b->cmap[a] < b->cmap[z]; });
  for (unsigned i = 0; i < C; i++)
    out[i] = make_uint2(order[i], b->cmap[order[i]]);
}

} // namespace

#include "fmd_batch_if.inc.hpp"      // launch_if_stage: the IF stage's kernel forms
#include "fmd_batch_process.inc.hpp" // submit_call: one call on the batch's streams, stage by stage
#include "fmd_scan.inc.hpp"          // fmd_scan_*: the band scan (its own object, the caller's stream)
#include "fmd_split.inc.hpp"         // fmd_split_*: the band splitter (its own object, the caller's stream)
#include "fmd_chan.inc.hpp"          // fmd_chan_*: the polyphase channeliser (likewise)

namespace
{

/* The carried regions of a channel: everything a call leaves behind for the next one, per channel.  A retuned
 * channel takes all of them from the silent twin (k_channel_restart); fmd_batch_debug_set "restart_skip" = index
 * leaves one out.  Both parities of a double-buffered region are copied: a restart runs when every earlier call
 * of the batch and of the twin is complete, so neither copy is being read.  What is NOT here is rewritten by
 * every call before it is read (demod, rlpf, rmf, alp, the half-band chain's tails, the status record) or is
 * batch-wide (positions, ring phases, the RDS oscillator sequence: the twin has the same ones). */
const char* const kRestartRegions[] = {
    "state",     // fstate, istate, r_data: every recurrence, meter and the RDS block assembly
    "if_hist",   // the IF FIR's delay line (tuned input samples), both hist_sel copies
    "br",        // the resampler's history rows of the baseband, both parities
    "mix",       // the first half-band stage's delay line (mixed rows), both parities
    "halfband",  // the delay lines of the later half-band / CIC stages
    "rds_lpf",   // the RDS low-pass ring (history rows of rdsraw), both parities
    "rds_mf",    // the matched filter ring (history rows of rpll)
    "audio_lpf", // the audio low-pass ring (history rows of rs), both parities
};
constexpr int kRestartRegionCount = int(sizeof(kRestartRegions) / sizeof(kRestartRegions[0]));

/* THE list of the carried regions of a batch with buffers of its own (or of the twin): group (index of
 * kRestartRegions), base, rows, element size, and the elements between two rows and between two channels.  Every
 * geometry gives the same entries in the same order, entries of no rows included (their users leave those out). */
struct CarriedRegion
{
  int group;
  void* base;
  unsigned rows, esz;
  size_t row, ch;
};
std::vector<CarriedRegion> carried_regions(const fmd_batch* x)
{
  const fmd::Design& d = x->des;
  std::vector<CarriedRegion> v;
  // time-major unless said otherwise: a row is CP elements, a channel's elements are neighbours
  auto add = [&](int group, void* base, size_t rows, unsigned esz, size_t row = 0, size_t ch = 1) {
    v.push_back(CarriedRegion{group, base, unsigned(rows), esz, row ? row : size_t(x->CP), ch});
  };
  add(0, x->fstate.p, fmd::F_SLOTS, 4);
  add(0, x->istate.p, fmd::I_SLOTS, 4);
  add(0, x->r_data.p, 4, 2);
  for (int q = 0; q < 2; q++) // channel-major: element j of channel c at c * if_order + j
    add(1, x->hist[q].p, d.if_order, 8, 1, d.if_order);
  for (int q = 0; q < 2; q++)
    add(2, x->brp(q), d.rs_order, 8);
  for (int q = 0; q < 2; q++)
    add(3, x->mix[q].p, d.hb[0].len - 1, 8);
  for (size_t s = 1; s < d.hb.size(); s++)
    add(4, x->hbbuf[s - 1].p, d.hb[s].len - 1, 8);
  for (int q = 0; q < 2; q++)
    add(5, x->rdsraw[q].p, d.rds_lpf_taps.size() - 1, 8);
  add(5, x->org.p, 1, 4); // ring origin: the twin's is 0, the batch phase
  add(6, x->rpll.p, d.rds_mf_taps.size() - 1, 4);
  add(6, x->org.p + x->CP, 1, 4);
  for (int q = 0; q < 2; q++)
    add(7, x->rs[q].p, d.lpf_taps.size() - 1, 8);
  return v;
}

/* restart_tab of a batch with buffers of its own, copying from the twin `tw` (one channel): its carried regions
 * paired with the twin's, entry by entry */
int build_restart_table(fmd_batch* x, const fmd_batch* tw)
{
  const fmd::Design& d = x->des;
  fmd::RestartTable& t = x->restart_tab;
  t.n = 0;
  const std::vector<CarriedRegion> mine = carried_regions(x), its = carried_regions(tw);
  bool bad = mine.size() != its.size();
  for (size_t i = 0; i < mine.size() && !bad; i++)
  {
    const CarriedRegion &m = mine[i], &w = its[i];
    bad = m.group != w.group || m.rows != w.rows || m.esz != w.esz || t.n >= fmd::kRestartMaxRegions;
    if (bad || m.rows == 0)
      continue;
    x->restart_group[t.n] = m.group;
    t.r[t.n++] = fmd::RestartRegion{m.base, w.base, m.rows, m.esz, m.row, m.ch, w.row};
  }
  if (bad)
    return fail(FMD_ERR_ARG, "fmd_batch_enable_retune: this geometry has more carried regions than the restart takes");
  // staging of the new tuner rows (the edit lists' is the batch's own): a slot per call index mod NSLOT, at most
  // one row per distinct shift
  const unsigned T = d.table_size;
  x->restart_rows_cap = std::min(2 * T - 1, x->C);
  const size_t rows_per_slot = size_t(x->restart_rows_cap) * T;
  if (x->d_rows.alloc(fmd_batch::NSLOT * rows_per_slot))
    return fail(FMD_ERR_DEVICE, "fmd_batch_enable_retune: device allocation failed");
  if (x->h_rows.alloc(fmd_batch::NSLOT * rows_per_slot))
    return fail(FMD_ERR_DEVICE, "fmd_batch_enable_retune: page-locked staging allocation failed");
  HIPCHK(x->edit_done.create());
  return FMD_OK;
}

/* `s` waits (on the device) for every call of x submitted so far; events already complete are left out */
hipError_t order_after_calls(fmd_batch* x, hipStream_t s)
{
  for (int q = 0; q < fmd_batch::NSLOT; q++)
  {
    if (x->slot_call[q] == 0)
      continue;
    for (int e : {fmd_batch::EV_INDONE, fmd_batch::EV_HEAVY, fmd_batch::EV_ROLL, fmd_batch::EV_RDS, fmd_batch::EV_AUD})
    {
      if (hipEventQuery(x->cev[q][e]) == hipSuccess)
        continue;
      (void)hipGetLastError(); // (hipErrorNotReady is an answer)
      if (hipError_t r = hipStreamWaitEvent(s, x->cev[q][e], 0))
        return r;
    }
  }
  return hipSuccess;
}

/* The pending edits of a batch with buffers of its own (plain or sub-batch), submitted in front of its next call:
 * on the stream its IF FIR will take, behind every earlier call of the batch (and of the twin, for restarts) -- so
 * no call in flight sees a changed byte, and every kernel of the next call (they all run behind its IF FIR) sees the
 * new state.  Edits of one channel apply in the order they were made: a retune replaces all the state a reset
 * clears (so a reset in front of it drops out), a reset behind a retune clears the restarted state again.  So the
 * restarts (k_channel_restart) go first, then the resets (k_channel_reset).  The twin's next call goes behind a
 * restart too (it reads the twin as the previous call left it). */
int submit_imports(fmd_batch* x, hipStream_t sF, const std::map<unsigned, int>& import_of); // fmd_batch_state.inc.hpp

int submit_edits(fmd_batch* x, fmd_batch* tw, hipStream_t stream)
{
  if (x->edits.empty())
    return FMD_OK;
  const bool serial_mode = x->concurrency == 0 || x->profiling >= 2;
  const hipStream_t sF = serial_mode ? stream : x->s_fir;
  const unsigned T = x->des.table_size;
  // what each edited channel ends up with.  The last retune's shift counts; a table row depends on the shift's
  // remainder as C++ takes it (sign included: make_tuner_lut reduces shift * i so, and the angles of s and s - T
  // are different floats), so there are at most 2 T - 1 distinct rows
  struct Fate
  {
    bool retune = false, reset = false;
    int shift = 0;
    int imp = -1; // the import the channel's state comes from (replaces all of it, like a retune)
  };
  std::map<unsigned, Fate> fate;
  for (const auto& e : x->edits)
  {
    Fate& f = fate[e.ch];
    if (e.reset)
      f.reset = true;
    else if (e.imp >= 0)
      f = Fate{false, false, 0, e.imp};
    else
      f = Fate{true, false, int((long long)(e.shift) % (long long)T), -1};
  }
  x->edits.clear();
  std::map<unsigned, int> import_of;
  for (const auto& [ch, f] : fate)
    if (f.imp >= 0)
      import_of[ch] = f.imp;
  const int slot = int(x->restart_seq++ % fmd_batch::NSLOT);
  HIPCHK(x->edit_ev[slot].sync_if_in_use()); // the copy of NSLOT edits ago (long done unless the caller never waits)
  int2* he = x->h_edits.p + size_t(slot) * 2 * x->C;
  float2* hr = x->h_rows.p ? x->h_rows.p + size_t(slot) * x->restart_rows_cap * T : nullptr;
  std::map<int, int> row_of; // shift % T -> row of the staging table
  unsigned n_rs = 0, n_z = 0;
  for (const auto& [ch, f] : fate) // channel order: the kernels' writes of one row go to neighbouring channels
  {
    if (!f.retune)
      continue;
    if (!tw) // (fmd_batch_retune_channels refuses a batch without a twin)
      return fail(FMD_ERR_STATE, "a retune of a batch without retuning enabled");
    auto it = row_of.find(f.shift);
    if (it == row_of.end())
    {
      const int r = int(row_of.size());
      it = row_of.emplace(f.shift, r).first;
      const auto lut = fmd::make_tuner_lut(T, f.shift);
      std::memcpy(hr + size_t(r) * T, lut.data(), size_t(T) * sizeof(float2));
    }
    he[n_rs++] = make_int2(int(ch), it->second);
  }
  for (const auto& [ch, f] : fate)
    if (f.reset)
      he[n_rs + n_z++] = make_int2(int(ch), 0);
  int2* de = x->d_edits.p + size_t(slot) * 2 * x->C;
  HIPCHK(order_after_calls(x, sF));
  if (n_rs)
    HIPCHK(order_after_calls(tw, sF));
  if (n_rs + n_z)
    HIPCHK(hipMemcpyAsync(de, he, (n_rs + n_z) * sizeof(int2), hipMemcpyHostToDevice, sF));
  float2* dr = nullptr;
  if (n_rs)
  {
    dr = x->d_rows.p + size_t(slot) * x->restart_rows_cap * T;
    HIPCHK(hipMemcpyAsync(dr, hr, row_of.size() * T * sizeof(float2), hipMemcpyHostToDevice, sF));
  }
  HIPCHK(x->edit_ev[slot].record_use(sF));
  if (n_rs)
  {
    fmd::RestartTable tab{};
    for (int i = 0; i < x->restart_tab.n; i++)
      if (x->restart_group[i] != x->restart_skip)
        tab.r[tab.n++] = x->restart_tab.r[i];
    // a few edits: one workgroup per region; all channels: ~8 rows of every region per workgroup and pass
    const unsigned blocks = std::min(64u, (n_rs * 8u + 255u) / 256u);
    hipLaunchKernelGGL(fmd::k_channel_restart, dim3(blocks, tab.n + 1), dim3(256), 0, sF, tab, (const int2*)de, n_rs,
                       (const float2*)dr, (float2*)x->lut.p, T);
    HIPCHK(hipGetLastError());
  }
  if (!x->imports.empty()) // behind the restarts, in front of the resets (a channel takes one of the two)
    if (int rc = submit_imports(x, sF, import_of))
      return rc;
  if (n_z)
  {
    fmd::ResetTable tab{};
    for (const fmd::ResetRegion& r : reset_regions(x))
    {
      if (tab.n >= fmd::kResetMaxRegions)
        return fail(FMD_ERR_ARG, "fmd_batch_reset_channels: more reset regions than k_channel_reset takes");
      tab.r[tab.n++] = r;
    }
    tab.CP = x->CP;
    tab.origin = x->org.p;
    // the next call's first RDS-rate sample is sample 0 of the reset channels' rings
    tab.org_lpf = x->dbg_reset_keep_phase ? 0u : x->rds_lpf_g;
    tab.org_mf = x->dbg_reset_keep_phase ? 0u : x->mf_g;
    const unsigned blocks = std::min(64u, (n_z * 8u + 255u) / 256u);
    hipLaunchKernelGGL(fmd::k_channel_reset, dim3(blocks, tab.n + 1), dim3(256), 0, sF, tab,
                       (const int2*)(de + n_rs), n_z);
    HIPCHK(hipGetLastError());
    x->origins_live = true;
  }
  if (n_rs && sF != tw->s_fir)
  {
    HIPCHK(hipEventRecord(x->edit_done, sF));
    HIPCHK(hipStreamWaitEvent(tw->s_fir, x->edit_done, 0));
  }
  return FMD_OK;
}

/* the shift channel c of the caller-facing batch b decodes with in call `ci` */
int shift_at(fmd_batch* b, unsigned c, uint32_t ci)
{
  std::lock_guard<std::mutex> lk(b->log_mu);
  int s = b->shifts[c];
  if (c < b->shift_log.size())
    for (const auto& [k, v] : b->shift_log[c])
      if (k <= ci)
        s = v;
  return s;
}

/* What the edits of channel c in front of the calls (epoch, ci] ask of its group decoder: 0 nothing; 1 a reset
 * (fmd_batch_reset_channels: cFmDecoder::Reset keeps the UECP sequence counter, the last PTY and the A/B flags); 2 a
 * new decoder (a retune: the decoder created with the new shift has a group decoder no group has reached, and a reset
 * of that one changes nothing).  *k_last: the last of those calls. */
int gdec_edit_between(fmd_batch* b, unsigned c, uint32_t epoch, uint32_t ci, uint32_t* k_last)
{
  std::lock_guard<std::mutex> lk(b->log_mu);
  *k_last = 0;
  if (c >= b->shift_log.size())
    return 0;
  for (const auto& [k, v] : b->shift_log[c])
    if (k <= ci)
      *k_last = k;
  if (*k_last <= epoch)
    return 0;
  if (c < b->retune_log.size())
    for (uint32_t k : b->retune_log[c])
      if (k > epoch && k <= *k_last)
        return 2;
  return 1;
}

/* The group decoder of channel c before a group of call ci: reset (a reset) or replaced by a new one (a retune) once
 * at the first group of a call at or behind an edit of the channel (groups of earlier calls, collected late, still
 * go through the old state). */
void gdec_follow_edits(fmd_batch* b, unsigned c, uint32_t ci)
{
  // the decoders of imported channels (fmd_batch_import_channels) whose first call has come, in call order
  if (auto it = b->gdec_imports.find(c); it != b->gdec_imports.end())
  {
    auto& v = it->second;
    while (!v.empty() && v.front().k <= ci)
    {
      b->gdec[c] = std::move(v.front().g);
      b->gdec_epoch[c] = std::max(b->gdec_epoch[c], v.front().k);
      v.erase(v.begin());
    }
    if (v.empty())
      b->gdec_imports.erase(it);
  }
  uint32_t k_last = 0;
  if (const int what = gdec_edit_between(b, c, b->gdec_epoch[c], ci, &k_last))
  {
    if (what == 2)
      b->gdec[c].reset(); // (the caller creates the new one with the first group)
    else if (b->gdec[c])
      b->gdec[c]->reset();
    b->gdec_epoch[c] = k_last;
  }
}

/* a retune or reset made behind an import of the same call: the imported group decoder never gets a group */
void drop_gdec_import(fmd_batch* b, unsigned c, uint32_t k)
{
  auto it = b->gdec_imports.find(c);
  if (it == b->gdec_imports.end())
    return;
  while (!it->second.empty() && it->second.back().k >= k)
    it->second.pop_back();
  if (it->second.empty())
    b->gdec_imports.erase(it);
}

/* input rows channel numbers may name: the map's, or the cpc rule's */
unsigned capture_rows(const fmd_batch* b)
{
  return b->map_on ? b->n_cap : b->C / b->cpc;
}

/* the capture channel c of the caller-facing batch b reads in its next call */
unsigned capture_at(fmd_batch* b, unsigned c)
{
  if (!b->map_on)
    return c / b->cpc;
  unsigned lc = 0;
  const fmd_batch* ob = owner_of(b, c, &lc);
  return ob->cmap[lc];
}

/* a list of distinct channels of b and their captures (either list may be absent) */
int check_channel_list(fmd_batch* b, const unsigned* channels, const unsigned* captures, unsigned n, const char* who)
{
  if (b->failed)
    return fail(FMD_ERR_ARG, std::string(who) + ": the batch has failed (fmd_batch_reset clears it)");
  std::vector<unsigned> seen(channels, channels + n);
  std::sort(seen.begin(), seen.end());
  if (n && seen.back() >= b->C)
    return fail(FMD_ERR_ARG, std::string(who) + ": channel " + std::to_string(seen.back()) + " out of range");
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
    return fail(FMD_ERR_ARG, std::string(who) + ": a channel is listed twice");
  const unsigned rows = capture_rows(b);
  for (unsigned i = 0; captures && i < n; i++)
    if (captures[i] >= rows)
      return fail(FMD_ERR_ARG, std::string(who) + ": capture " + std::to_string(captures[i]) + " out of range (" +
                                   std::to_string(rows) + " captures)");
  return FMD_OK;
}

/* Turns the cpc rule into the same map where there is none yet (fmd_batch_switch_captures on such a batch): the walk
 * staging of every batch with buffers of its own, its channels' rows.  Calls in flight keep the plain form. */
int ensure_map(fmd_batch* b, const char* who)
{
  if (b->map_on)
    return FMD_OK;
  HIPCHK(hipSetDevice(b->device));
  const std::vector<Part> ps = parts(b);
  for (const Part& p : ps)
  {
    fmd_batch* x = p.x;
    if (x->d_walk.n < x->C && x->d_walk.alloc(x->C))
      return fail(FMD_ERR_DEVICE, std::string(who) + ": device allocation failed");
    if (x->h_walk.n < size_t(fmd_batch::NSLOT) * x->C && x->h_walk.alloc(size_t(fmd_batch::NSLOT) * x->C))
      return fail(FMD_ERR_DEVICE, std::string(who) + ": page-locked staging allocation failed");
    for (Event& e : x->walk_ev)
      if (!e.e)
        HIPCHK(e.create());
  }
  const unsigned rows = b->C / b->cpc;
  for (const Part& p : ps)
  {
    fmd_batch* x = p.x;
    x->cmap.resize(x->C);
    for (unsigned c = 0; c < x->C; c++)
      x->cmap[c] = (p.ch0 + c) / b->cpc;
    x->map_on = true;
    x->map_dirty = true;
    x->n_cap = rows;
  }
  b->map_on = true;
  b->n_cap = rows;
  return FMD_OK;
}

} // namespace

extern "C" {

static int wait_impl(fmd_batch* b, int lag, void* stream_, bool take_lost);

/* One call of any batch: a plain one directly; a shell's as one call of every sub-batch, in channel order, on the
 * same streams (fmd_batch::subs). */
static int process_shell(fmd_batch* b, const Call& c);

/* Pending single-channel edits (retunes, resets) in front of the call; with retuning enabled, the silent twin's call
 * (zeros of the same size, on the same streams) behind it.  A batch with neither takes the plain path alone. */
static int process_any(fmd_batch* b, const Call& c)
{
  if (!b || (!b->twin && !b->edits_pending))
    return process_shell(b, c);
  fmd::CallPlan pl;
  if (int rc = check_call(b, c, pl))
    return rc;
  fmd_batch* tw = b->twin.get();
  for (const Part& p : parts(b))
    if (int rc = submit_edits(p.x, tw, static_cast<hipStream_t>(c.stream)))
    {
      mark_failed(b, "a channel edit could not be submitted");
      return rc;
    }
  b->edits_pending = false;
  const int rc = process_shell(b, c);
  if (rc != FMD_OK || !tw)
    return rc;
  // (the twin's audio is discarded: it stays float whatever the call's format; its multiplex is not written at all,
  // and it has no feed)
  Call t;
  t.iq = b->twin_iq.p;
  t.samples = c.samples;
  if (c.ciq_in()) // (the twin takes the call's kind: M float pairs of the same zeros, every channel the one row)
    t.iq_fmt = FMD_IN_CIQ_F32;
  t.audio.p = b->twin_audio.p;
  t.audio.stride = b->twin_audio.n;
  t.stream = c.stream;
  const int trc = submit_call(tw, t);
  if (trc != FMD_OK)
    mark_failed(b, "the silent twin refused a call the batch took");
  return trc;
}

static int process_shell(fmd_batch* b, const Call& c)
{
  if (!b || b->subs.empty())
    return submit_call(b, c);
  fmd::CallPlan pl;
  if (int rc = check_call(b, c, pl))
    return rc;
  unsigned nf = 0;
  for (size_t k = 0; k < b->subs.size(); k++)
  {
    fmd_batch* sb = b->subs[k].get();
    const unsigned ch0 = b->sub_ch0[k];
    sb->sched_prev2 = b->vheavy[1];
    Call sc = c;
    // (a capture map: every sub-batch takes the first row, its walk names the rows it reads)
    // (channel IQ rows: one per channel whatever the map)
    const size_t row0 = c.ciq_in() ? ch0 : b->map_on ? 0 : ch0 / b->cpc;
    sc.iq = static_cast<const char*>(c.iq) + row0 * c.iq_stride * c.in_esz();
    // (the sub-batch's first row of every output; every sub-batch counts the feed's frames for itself)
    for (FormatKind k : kOutKinds)
      sc.out(k) = c.out(k).from_channel(ch0, b->sel[k].on);
    sc.audio.out = &nf;
    const int rc = submit_call(sb, sc);
    if (rc != FMD_OK)
    { // the first sub-batch refuses what every one of them would refuse (same geometry, same positions): nothing
      // has been submitted.  Later: part of the call is on the device -- the batch is unusable until reset.
      if (k > 0)
      {
        b->failed = true;
        b->fail_msg = std::string("a call broke off between two sub-batches: ") + g_err;
      }
      return rc;
    }
    b->vheavy[1] = b->vheavy[0];
    b->vheavy[0] = sb->cev[sb->call_index % fmd_batch::NSLOT][fmd_batch::EV_HEAVY];
  }
  b->call_index = b->subs[0]->call_index;
  b->lastM = b->subs[0]->lastM;
  b->lastA = b->subs[0]->lastA;
  b->lastR = b->subs[0]->lastR;
  if (c.audio.out)
    *c.audio.out = nf;
  if (b->concurrency == 1) // the caller's stream is ordered after every call (the sub-batches run in mode 2)
    return wait_impl(b, 0, c.stream, false);
  return FMD_OK;
}

/* A call as the entry points take it: the input, the audio rows and the stream (mpx and feed: the entry point's). */
static Call make_call(const void* iq, int iq_format, size_t iq_stride, unsigned samples, void* audio, int pcm_format,
                      size_t audio_stride, unsigned* out_samples, void* stream = nullptr)
{
  Call c;
  c.iq = iq;
  c.iq_fmt = iq_format;
  c.iq_stride = iq_stride;
  c.samples = samples;
  c.audio = Out{FMT_PCM, audio, pcm_format, audio_stride, out_samples};
  c.stream = stream;
  return c;
}

/* What an entry point `who` checks of its arguments before the call goes on, for all of them in one order -- the
 * formats; then WAY_DEVICE: the pointers and strides the kernels store through, WAY_HOST: what the staged copy needs
 * (no alignment; a stride only between rows), WAY_FORMATS: nothing more (fmd_process_stream_*: the decoder comes
 * next).  Checks of an output apply only when its pointer is given and, for the multiplex, its selection is not
 * empty (the channel IQ: likewise; a feed selection of no rows still counts the feed's frames).  Clears the out-counts a refused call would
 * leave behind, drops the multiplex of a selection of no rows, and says whether the feed is delivered.  No HIP call
 * in here: the refusals hold without a device. */
enum CallWay { WAY_DEVICE, WAY_HOST, WAY_FORMATS };
static int check_call_args(const char* who, CallWay way, fmd_batch* b, Call& c)
{
  auto refuse = [&](int code, const char* what) { return fail(code, std::string(who) + ": " + what); };
  if (!format_ok(FMT_CIQ, c.ciq.fmt))
    return refuse(FMD_ERR_ARG, kFormats[FMT_CIQ].must);
  if (c.ciq.out)
    *c.ciq.out = 0;
  if (!format_ok(FMT_FEED, c.feed.fmt))
    return refuse(FMD_ERR_ARG, kFormats[FMT_FEED].must);
  if (c.feed.out)
    *c.feed.out = 0;
  if (!format_ok(FMT_MPX, c.mpx.fmt))
    return refuse(FMD_ERR_ARG, kFormats[FMT_MPX].must);
  if (ciq_in_format(c.iq_fmt) && !c.from_record)
    return refuse(FMD_ERR_ARG, kCiqInOnlyCall);
  if (!format_ok(FMT_IQ, c.iq_fmt) && !c.ciq_in())
    return refuse(FMD_ERR_ARG, c.from_record ? "iq_format must be one of FMD_IQ_F32, _U8, _S8, _S16 (0..3) or "
                                               "FMD_IN_CIQ_F32, _S16 (32, 33)"
                                             : kFormats[FMT_IQ].must);
  if (!format_ok(FMT_PCM, c.audio.fmt))
    return refuse(FMD_ERR_ARG, kFormats[FMT_PCM].must);
  if (way == WAY_FORMATS)
    return FMD_OK;
  const bool dev = way == WAY_DEVICE;
  // a lane stores 16 bytes of a row at a time: every row has to start on a 16-byte boundary
  if (dev && c.feed.p && !c.feed.rows_aligned())
    return refuse(FMD_ERR_ARG, "the feed pointer must be 16-byte aligned and feed_channel_stride a multiple of 4 "
                               "(FMD_FEED_F32) / 8 (FMD_FEED_S16) elements");
  // channel IQ rows as input: a lane loads 16 bytes of a row at a time, the rule of the ciq output's rows
  if (dev && c.ciq_in() && c.iq && ((reinterpret_cast<uintptr_t>(c.iq) % 16) || (c.iq_stride * c.in_esz()) % 16))
    return refuse(FMD_ERR_ARG, "with FMD_IN_CIQ_* the iq pointer must be 16-byte aligned and iq_channel_stride a "
                               "multiple of 2 (FMD_IN_CIQ_F32) / 4 (FMD_IN_CIQ_S16) complex samples");
  // (a device call's other null arguments get their own sentence further down)
  if (!b || (!dev && (!c.iq || (!c.audio.p && audio_rows_due(b)))))
    return refuse(FMD_ERR_ARG, "null argument");
  if (c.feed.p && !b->feed_div)
    return refuse(FMD_ERR_STATE, "a feed pointer while the feed is off (fmd_batch_set_feed turns it on)");
  // ... one row per channel, `samples` = M complex samples each
  if (c.ciq_in() && b->C > 1 && c.iq_stride < c.samples)
    return refuse(FMD_ERR_ARG, "with FMD_IN_CIQ_* iq_channel_stride must be at least samples, the call's baseband "
                               "length: one row per channel");
  // four 16-bit frames go out as one 16-byte store: every row has to start on a 16-byte boundary
  if (dev && c.audio.fmt == FMD_PCM_S16 && c.iq && c.audio.p && !c.audio.rows_aligned())
    return refuse(FMD_ERR_ARG, "for FMD_PCM_S16 the audio pointer must be 16-byte aligned and audio_channel_stride a "
                               "multiple of 8 elements");
  auto rows_of = [b](FormatKind k) { return b->sel[k].on ? b->sel[k].n_total : b->C; };
  const unsigned m_rows = rows_of(FMT_MPX), f_rows = rows_of(FMT_FEED);
  if (m_rows == 0) // a selection of no rows: the call without the multiplex
    c.mpx.p = nullptr;
  if (c.mpx.out)
    *c.mpx.out = 0;
  c.feed.deliver = f_rows != 0;
  const unsigned q_rows = rows_of(FMT_CIQ);
  if (q_rows == 0) // a selection of no rows: the call without the channel IQ
    c.ciq.p = nullptr;
  if (!c.mpx.p && !c.feed.p && !c.ciq.p)
    return FMD_OK;
  // the rows hold the call's samples -- looked at here, in front of the pending channel edits: a refused call leaves
  // the batch as it was (a call refused for its size has no samples: check_call has the sentence)
  fmd::CallPlan pl;
  (void)plan_of_call(b, c, pl);
  if (c.mpx.p && dev && !c.mpx.rows_aligned())
    return refuse(FMD_ERR_ARG, "the multiplex pointer must be 16-byte aligned and mpx_channel_stride a multiple of 4 "
                               "(FMD_MPX_F32) / 8 (FMD_MPX_S16) elements");
  if (c.mpx.p && (dev || m_rows > 1) && c.mpx.stride < pl.M)
    return refuse(FMD_ERR_ARG, "mpx_channel_stride smaller than the call's baseband length "
                               "(fmd_batch_max_mpx_samples is the bound)");
  if (c.feed.p && (dev || f_rows > 1) && c.feed.stride < pl.feed_n)
    return refuse(FMD_ERR_ARG, "feed_channel_stride smaller than the call's feed samples "
                               "(fmd_batch_max_feed_samples is the bound)");
  if (c.ciq.p && dev && !c.ciq.rows_aligned())
    return refuse(FMD_ERR_ARG, "the ciq pointer must be 16-byte aligned and ciq.stride a multiple of 2 (FMD_CIQ_F32) / "
                               "4 (FMD_CIQ_S16) complex samples");
  if (c.ciq.p && (dev || q_rows > 1) && c.ciq.stride < pl.M)
    return refuse(FMD_ERR_ARG, "ciq.stride smaller than the call's baseband length (fmd_batch_max_mpx_samples is the "
                               "bound)");
  return FMD_OK;
}

static int process_device_checked(const char* who, fmd_batch* b, Call& c)
{
  if (int rc = check_call_args(who, WAY_DEVICE, b, c))
    return rc;
  return process_any(b, c);
}

int fmd_batch_process_device_pcm(fmd_batch* b, const void* d_iq, int iq_format, size_t iq_channel_stride,
                                 unsigned samples, void* d_audio, int pcm_format, size_t audio_channel_stride,
                                 unsigned* out_samples, void* stream)
{
  Call c = make_call(d_iq, iq_format, iq_channel_stride, samples, d_audio, pcm_format, audio_channel_stride,
                     out_samples, stream);
  return process_device_checked("fmd_batch_process_device_pcm", b, c);
}

int fmd_batch_process_device_mpx(fmd_batch* b, const void* d_iq, int iq_format, size_t iq_channel_stride,
                                 unsigned samples, void* d_audio, int pcm_format, size_t audio_channel_stride,
                                 unsigned* out_samples, void* d_mpx, int mpx_format, size_t mpx_channel_stride,
                                 unsigned* out_mpx_samples, void* stream)
{
  Call c = make_call(d_iq, iq_format, iq_channel_stride, samples, d_audio, pcm_format, audio_channel_stride,
                     out_samples, stream);
  c.mpx = Out{FMT_MPX, d_mpx, mpx_format, mpx_channel_stride, out_mpx_samples};
  return process_device_checked("fmd_batch_process_device_mpx", b, c);
}

int fmd_batch_process_device_feed(fmd_batch* b, const void* d_iq, int iq_format, size_t iq_channel_stride,
                                  unsigned samples, void* d_audio, int pcm_format, size_t audio_channel_stride,
                                  unsigned* out_samples, void* d_mpx, int mpx_format, size_t mpx_channel_stride,
                                  unsigned* out_mpx_samples, void* d_feed, int feed_format, size_t feed_channel_stride,
                                  unsigned* out_feed_samples, void* stream)
{
  Call c = make_call(d_iq, iq_format, iq_channel_stride, samples, d_audio, pcm_format, audio_channel_stride,
                     out_samples, stream);
  c.mpx = Out{FMT_MPX, d_mpx, mpx_format, mpx_channel_stride, out_mpx_samples};
  c.feed = Out{FMT_FEED, d_feed, feed_format, feed_channel_stride, out_feed_samples};
  return process_device_checked("fmd_batch_process_device_feed", b, c);
}

/* The call record of the C ABI as the internal one (the _call entry points): null and size first. */
static int call_of_record(const char* who, const fmd_call* r, Call& c)
{
  if (!r)
    return fail(FMD_ERR_ARG, std::string(who) + ": null call record");
  if (r->size != sizeof(fmd_call))
    return fail(FMD_ERR_ARG, std::string(who) + ": call->size must be sizeof(fmd_call)");
  auto rows = [](FormatKind k, const fmd_rows& o) { return Out{k, o.p, o.format, o.stride, o.count}; };
  c.iq = r->iq;
  c.iq_fmt = r->iq_format;
  c.iq_stride = r->iq_channel_stride;
  c.samples = r->samples;
  c.audio = rows(FMT_PCM, r->audio);
  c.mpx = rows(FMT_MPX, r->mpx);
  c.feed = rows(FMT_FEED, r->feed);
  c.ciq = rows(FMT_CIQ, r->ciq);
  c.stream = r->stream;
  c.from_record = true;
  return FMD_OK;
}

int fmd_batch_process_device_call(fmd_batch* b, const fmd_call* call)
{
  Call c;
  if (int rc = call_of_record("fmd_batch_process_device_call", call, c))
    return rc;
  return process_device_checked("fmd_batch_process_device_call", b, c);
}

int fmd_batch_process_device_fmt(fmd_batch* b, const void* d_iq, int format, size_t iq_channel_stride,
                                 unsigned samples, float* d_audio, size_t audio_channel_stride,
                                 unsigned* out_floats, void* stream)
{
  if (!format_ok(FMT_IQ, format))
    return fail(FMD_ERR_ARG, "fmd_batch_process_device_fmt: format must be one of FMD_IQ_F32, _U8, _S8, _S16 (0..3)");
  return fmd_batch_process_device_pcm(b, d_iq, format, iq_channel_stride, samples, d_audio, FMD_PCM_F32,
                                      audio_channel_stride, out_floats, stream);
}

int fmd_batch_process_device(fmd_batch* b, const float* d_iq, size_t iq_channel_stride,
                             unsigned samples, float* d_audio, size_t audio_channel_stride,
                             unsigned* out_floats, void* stream)
{
  return fmd_batch_process_device_fmt(b, d_iq, FMD_IQ_F32, iq_channel_stride, samples, d_audio, audio_channel_stride,
                                      out_floats, stream);
}

int fmd_batch_process_device_u8(fmd_batch* b, const uint8_t* d_iq_u8, size_t iq_channel_stride,
                                unsigned samples, float* d_audio, size_t audio_channel_stride,
                                unsigned* out_floats, void* stream)
{
  return fmd_batch_process_device_fmt(b, d_iq_u8, FMD_IQ_U8, iq_channel_stride, samples, d_audio,
                                      audio_channel_stride, out_floats, stream);
}

/* slots whose call is at least `lag` calls old (lag 0 = every call submitted so far) */
static bool slot_eligible(const fmd_batch* b, int q, int lag)
{
  return b->slot_call[q] != 0 && b->slot_call[q] + uint32_t(lag) <= b->call_index;
}

/* take_lost = false: the recoverable flag (groups lost) stays for whoever reports it */
static int wait_impl(fmd_batch* b, int lag, void* stream_, bool take_lost)
{
  if (!b || lag < 0 || lag > 4)
    return fail(FMD_ERR_ARG, "fmd_batch_wait: bad argument (lag must be 0..4)");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK(hipSetDevice(b->device));
  if (is_shell(b))
  {
    for (auto& sb : b->subs)
    {
      const int rc = wait_impl(sb.get(), lag, stream_, false);
      if (rc < 0)
        return check_device_errors(b); // (marks the shell failed too)
    }
    if (int rc = check_device_errors(b))
      return rc;
    return take_lost ? take_lost_groups(b) : FMD_OK;
  }
  /* Only events that have not completed yet become waits of the caller's stream: a completed event orders nothing.
   * (Until round 6 every wait went through all eligible slots -- up to 32 barrier packets per step in the caller's
   * queue, nearly all for calls long complete.  On the null stream that cost nothing measurable; on a stream of the
   * caller's own the command processor's work on them cost 4-7 % of the whole path: tools/node_bench 275 000 against
   * 288 000 MS/s on the null stream, bench.py --side-stream 264 000 against 284 000; docs/MEASUREMENTS.md, round 6.) */
  auto wait_if_pending = [&](hipEvent_t e) {
    if (hipEventQuery(e) == hipSuccess)
      return hipSuccess;
    (void)hipGetLastError(); // (hipErrorNotReady is not an error)
    return hipStreamWaitEvent(stream, e, 0);
  };
  for (int q = 0; q < fmd_batch::NSLOT; q++)
    if (slot_eligible(b, q, lag))
    {
      HIPCHK(wait_if_pending(b->cev[q][fmd_batch::EV_AUD]));
      HIPCHK(wait_if_pending(b->cev[q][fmd_batch::EV_RDS]));
      HIPCHK(wait_if_pending(b->cev[q][fmd_batch::EV_INDONE]));
      // the history rolls behind the heavy part (br, mix, half-band tails) belong to the call too
      HIPCHK(wait_if_pending(b->cev[q][fmd_batch::EV_ROLL]));
    }
  // asynchronous: reports what the device has flagged so far (calls that have finished)
  if (int rc = check_device_errors(b))
    return rc;
  return take_lost ? take_lost_groups(b) : FMD_OK;
}

int fmd_batch_wait_lagged(fmd_batch* b, int lag, void* stream_)
{
  return wait_impl(b, lag, stream_, true);
}

int fmd_batch_take_rds_lost(fmd_batch* b)
{
  if (!b)
    return fail(FMD_ERR_ARG, "null batch");
  return take_lost_groups(b) == FMD_WARN_RDS_LOST ? 1 : 0;
}

int fmd_batch_debug_set_spin_limit(fmd_batch* b, unsigned limit)
{
  if (!b)
    return fail(FMD_ERR_ARG, "null batch");
  set_all(b, &fmd_batch::spin_limit, limit);
  b->st.spin_limit = limit;
  for (auto& sb : b->subs)
    sb->st.spin_limit = limit;
  return FMD_OK;
}

int fmd_batch_debug_restart_skip(fmd_batch* b, int region)
{
  if (!b)
    return fail(FMD_ERR_ARG, "null batch");
  if (region < -1 || region >= kRestartRegionCount)
  {
    std::string names;
    for (const char* r : kRestartRegions)
      names += std::string(names.empty() ? "" : ", ") + r;
    return fail(FMD_ERR_ARG, "fmd_batch_debug_restart_skip: -1 or the index of a region (" + names + ")");
  }
  set_all(b, &fmd_batch::restart_skip, region);
  return FMD_OK;
}

int fmd_batch_debug_reset_keep_ring_phase(fmd_batch* b, int on)
{
  if (!b)
    return fail(FMD_ERR_ARG, "null batch");
  set_all(b, &fmd_batch::dbg_reset_keep_phase, on != 0);
  return FMD_OK;
}

int fmd_batch_debug_host_ms(fmd_batch* b, float out[4])
{
  if (!b || !out)
    return fail(FMD_ERR_ARG, "null argument");
  const unsigned n = b->host_calls;
  for (int i = 0; i < 4; i++)
  {
    out[i] = n ? float(b->host_ms[i] / n) : 0.0f;
    b->host_ms[i] = 0.0;
  }
  b->host_calls = 0;
  return int(n);
}

int fmd_batch_debug_set(fmd_batch* b, const char* key, int value)
{
  if (!b || !key)
    return fail(FMD_ERR_ARG, "null argument");
  const std::string k(key);
  // Keys move work between streams and change kernel forms: nothing of an earlier call may still be
  // running when the next call takes the new route -- drain the device first.
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  if (is_shell(b))
  { // every sub-batch takes the key
    for (auto& sb : b->subs)
      if (int rc = fmd_batch_debug_set(sb.get(), key, value))
        return rc;
    return FMD_OK;
  }
  if (k == "resampler")
  {
    if (value > 0 && b->rsr_R == 0)
      return fail(FMD_ERR_ARG, "fmd_batch_debug_set: no form of k_resample_ring fits this geometry");
    b->rsr_mode = value < 0 ? -1 : (value ? 1 : 0);
  }
  else if (k == "fir_nt")
    b->dbg_fir_nt = std::max(0, value);
  else if (k == "serial_claim")
    b->dbg_serial_claim = value != 0;
  else if (k == "serial_exclusive")
    b->serial_exclusive = value != 0;
  else if (k == "split_post")
    b->split_post = value != 0;
  else if (k == "hb4")
    b->dbg_hb4 = value != 0;
  else if (k == "ring4")
    b->dbg_ring4 = value != 0;
  else if (k == "lpf_late")
    b->dbg_lpf_late = value < 0 ? -1 : std::min(value, 2);
  else if (k == "stage_mask")
    b->dbg_stage_mask = value & 63;
  else if (k == "fir_ro")
  { // (-2: 2 with every tile on the edge path, the one body a tile had before the interior one; -3 is 3, which has
    // the edge body only.  The sign of this key and not a key `fir_interior`: the keys are held to 14)
    const int ro = value < 0 ? -value : value;
    b->dbg_fir_ro = (ro == 2 || ro == 3) ? ro : 1;
    b->dbg_fir_interior = value >= 0;
  }
  else if (k == "serial_probe")
  { // per-workgroup timing of the serial stage's last 8 launches (fmd_batch_debug_serial_probe)
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());
    b->serial_probe.release();
    if (value && b->serial_probe.alloc(size_t(8) * 3 * (b->CP / 64)))
      return fail(FMD_ERR_DEVICE, "serial probe allocation failed");
  }
  else if (k == "halfband_chain") // -1 the library decides, 0 a launch per stage, 1 k_halfband_chain wherever it applies
  {
    b->hbf_mode = value < 0 ? -1 : (value ? 1 : 0);
    // before the first call a small batch can still start the batch-wide oscillator sequence (and with it
    // the form of the serial stage that writes no mixed rows); later its chain reads mixed rows
    if (value > 0 && b->call_index == 0 && b->h_osc.p && b->des.hb.size() == 3 &&
        b->des.hb[0].len - 1 <= int(fmd_batch::kOscH))
      b->osc_on = true;
  }
  else if (k == "nomix") // 0: the serial stage writes the mixed rows also where k_halfband_chain follows
    b->dbg_nomix = value != 0;
  else if (k == "rsr_form") // 0: 2 outputs x 8 waves, 1: 4 x 4, 2: 2 x 4 (falls through to the next that fits)
  {
    bool ok = false;
    for (int f = std::max(0, std::min(2, value)); f < 3 && !ok; f++)
      ok = rsr_configure(b, f);
  }
  else
    return fail(FMD_ERR_ARG, "fmd_batch_debug_set: unknown key '" + k + "'");
  return FMD_OK;
}

int fmd_batch_enable_retune(fmd_batch* b)
{
  if (!b)
    return fail(FMD_ERR_ARG, "fmd_batch_enable_retune: null batch");
  if (b->twin)
    return FMD_OK;
  if (b->call_index != 0)
    return fail(FMD_ERR_STATE, "fmd_batch_enable_retune: only before the batch's first call");
  HIPCHK(hipSetDevice(b->device));
  // the twin: one channel of the same geometry on this batch's streams (a shell's: the ones its sub-batches share)
  fmd_batch* tw = nullptr;
  const int zero_shift = 0;
  if (int rc = create_one(&b->cparams, 1, &zero_shift, b->device, nullptr, nullptr, b, &tw))
    return rc;
  std::unique_ptr<fmd_batch> twin(tw);
  twin->concurrency = 2; // ordered by the restarts that read it, never by the caller's stream
  if (b->twin_iq.alloc(FMD_MAX_BLOCK) || b->twin_audio.alloc(fmd_batch_max_audio_floats(tw, FMD_MAX_BLOCK)))
    return fail(FMD_ERR_DEVICE, "fmd_batch_enable_retune: device allocation failed");
  for (const Part& p : parts(b))
    if (int rc = build_restart_table(p.x, tw))
      return rc;
  HIPCHK(hipDeviceSynchronize());
  {
    std::lock_guard<std::mutex> lk(b->log_mu);
    b->shift_log.resize(b->C); // (resets made before the first call may have started it)
  }
  b->gdec_epoch.resize(b->C, 0u);
  b->twin = std::move(twin);
  return FMD_OK;
}

int fmd_batch_retune_channels(fmd_batch* b, const unsigned* channels, const int* shifts, unsigned n)
{
  if (!b || !channels || !shifts)
    return fail(FMD_ERR_ARG, "fmd_batch_retune_channels: null argument");
  if (b->failed)
    return fail(FMD_ERR_ARG, "fmd_batch_retune_channels: the batch has failed (fmd_batch_reset clears it)");
  if (!b->twin)
    return fail(FMD_ERR_STATE, "fmd_batch_retune_channels: retuning is not enabled (fmd_batch_enable_retune)");
  if (int rc = check_channel_list(b, channels, nullptr, n, "fmd_batch_retune_channels"))
    return rc;
  const uint32_t k = b->call_index + 1; // the call the edit takes effect at
  std::lock_guard<std::mutex> lk(b->log_mu);
  for (unsigned i = 0; i < n; i++)
  {
    unsigned lc = 0;
    fmd_batch* ob = owner_of(b, channels[i], &lc);
    ob->edits.push_back(fmd_batch::Edit{lc, shifts[i], false});
    drop_gdec_import(b, channels[i], k);
    auto& log = b->shift_log[channels[i]];
    if (!log.empty() && log.back().first == k)
      log.back().second = shifts[i];
    else
      log.emplace_back(k, shifts[i]);
    if (b->retune_log.size() < b->C)
      b->retune_log.resize(b->C);
    auto& rlog = b->retune_log[channels[i]];
    if (rlog.empty() || rlog.back() != k)
      rlog.push_back(k);
  }
  b->edits_pending = true;
  return FMD_OK;
}

int fmd_batch_reset_channels(fmd_batch* b, const unsigned* channels, unsigned n)
{
  if (!b || !channels)
    return fail(FMD_ERR_ARG, "fmd_batch_reset_channels: null argument");
  if (b->failed)
    return fail(FMD_ERR_ARG, "fmd_batch_reset_channels: the batch has failed (fmd_batch_reset clears it)");
  std::vector<unsigned> seen(channels, channels + n);
  std::sort(seen.begin(), seen.end());
  if (n && seen.back() >= b->C)
    return fail(FMD_ERR_ARG, "fmd_batch_reset_channels: channel " + std::to_string(seen.back()) + " out of range");
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
    return fail(FMD_ERR_ARG, "fmd_batch_reset_channels: a channel is listed twice");
  if (n == 0)
    return FMD_OK;
  const uint32_t k = b->call_index + 1; // the call the edit takes effect at
  std::lock_guard<std::mutex> lk(b->log_mu);
  if (b->shift_log.empty())
  {
    b->shift_log.resize(b->C);
    b->gdec_epoch.assign(b->C, 0u);
  }
  for (unsigned i = 0; i < n; i++)
  {
    unsigned lc = 0;
    fmd_batch* ob = owner_of(b, channels[i], &lc);
    ob->edits.push_back(fmd_batch::Edit{lc, 0, true});
    drop_gdec_import(b, channels[i], k);
    // the log marks the call for the group decoder; the shift stays what it is
    auto& log = b->shift_log[channels[i]];
    if (log.empty() || log.back().first != k)
      log.emplace_back(k, log.empty() ? b->shifts[channels[i]] : log.back().second);
  }
  b->edits_pending = true;
  return FMD_OK;
}

int fmd_batch_wait(fmd_batch* b, void* stream_)
{
  return fmd_batch_wait_lagged(b, 0, stream_);
}

int fmd_batch_set_channels_per_capture(fmd_batch* b, unsigned channels_per_capture)
{
  if (!b)
    return fail(FMD_ERR_ARG, "null batch");
  const unsigned k = channels_per_capture ? channels_per_capture : 1u;
  if (b->C % k)
    return fail(FMD_ERR_ARG, "fmd_batch_set_channels_per_capture: the channel count is not a multiple of it");
  for (size_t i = 0; i < b->subs.size(); i++) // a capture's channels must not straddle two sub-batches
    if (b->sub_ch0[i] % k || b->subs[i]->C % k)
      return fail(FMD_ERR_ARG, "fmd_batch_set_channels_per_capture: with " + std::to_string(b->C) +
                                   " channels the batch runs as sub-batches of " + std::to_string(b->subs[0]->C) +
                                   ", which is not a multiple of it");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  set_all(b, &fmd_batch::cpc, k);
  // the contiguous rule replaces any capture map
  set_all(b, &fmd_batch::map_on, false);
  set_all(b, &fmd_batch::n_cap, 0u);
  return FMD_OK;
}


int fmd_batch_set_capture_map(fmd_batch* b, const unsigned* capture_of_channel, unsigned n_captures)
{
  if (!b)
    return fail(FMD_ERR_ARG, "fmd_batch_set_capture_map: null batch");
  if (capture_of_channel)
  {
    if (n_captures == 0)
      return fail(FMD_ERR_ARG, "fmd_batch_set_capture_map: no captures");
    for (unsigned c = 0; c < b->C; c++)
      if (capture_of_channel[c] >= n_captures)
        return fail(FMD_ERR_ARG, "fmd_batch_set_capture_map: channel " + std::to_string(c) + " reads capture " +
                                     std::to_string(capture_of_channel[c]) + " of " + std::to_string(n_captures));
  }
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  if (!capture_of_channel) // one row per channel, as after creation
    return fmd_batch_set_channels_per_capture(b, 1);
  set_all(b, &fmd_batch::cpc, 1u);
  if (int rc = ensure_map(b, "fmd_batch_set_capture_map"))
    return rc;
  for (const Part& p : parts(b))
  {
    std::copy(capture_of_channel + p.ch0, capture_of_channel + p.ch0 + p.x->C, p.x->cmap.begin());
    p.x->map_dirty = true;
  }
  set_all(b, &fmd_batch::n_cap, n_captures);
  return FMD_OK;
}

int fmd_batch_debug_capture_walk(fmd_batch* b, int on)
{
  if (!b)
    return fail(FMD_ERR_ARG, "fmd_batch_debug_capture_walk: null batch");
  set_all(b, &fmd_batch::capture_walk, on != 0);
  for (const Part& p : parts(b)) // the next call takes the walk in the new order (calls in flight keep theirs: the
    p.x->map_dirty = p.x->map_on; // copy is ordered like a switch)
  return FMD_OK;
}

int fmd_batch_get_capture_map(fmd_batch* b, unsigned* out, unsigned cap)
{
  if (!b || (cap && !out))
    return fail(FMD_ERR_ARG, "fmd_batch_get_capture_map: null argument");
  for (unsigned c = 0; c < std::min(cap, b->C); c++)
    out[c] = capture_at(b, c);
  return int(capture_rows(b));
}

int fmd_batch_switch_captures(fmd_batch* b, const unsigned* channels, const unsigned* captures, unsigned n)
{
  if (!b || !channels || !captures)
    return fail(FMD_ERR_ARG, "fmd_batch_switch_captures: null argument");
  if (int rc = check_channel_list(b, channels, captures, n, "fmd_batch_switch_captures"))
    return rc;
  if (n == 0)
    return FMD_OK;
  if (int rc = ensure_map(b, "fmd_batch_switch_captures"))
    return rc;
  for (unsigned i = 0; i < n; i++)
  {
    unsigned lc = 0;
    fmd_batch* ob = owner_of(b, channels[i], &lc);
    ob->cmap[lc] = captures[i];
    ob->map_dirty = true;
  }
  return FMD_OK;
}

/* fmd_batch_select_audio / _mpx: checked as a whole, then every batch with buffers takes its part -- (local channel,
 * global row), sorted by channel: the audio table is indexed by channel anyway, and the multiplex writer's gathers
 * coalesce over neighbouring channels -- and builds a new table version in front of its next call (sel_table). */
static int select_rows(fmd_batch* b, FormatKind kind, const unsigned* channels, unsigned n, const char* who)
{
  if (!b)
    return fail(FMD_ERR_ARG, std::string(who) + ": null batch");
  if (b->decoder_owned)
    return fail(FMD_ERR_STATE, std::string(who) + ": the batch behind an fmd_decoder takes no selection (the decoder "
                                                  "owns its output)");
  if (b->failed)
    return fail(FMD_ERR_ARG, std::string(who) + ": the batch has failed (fmd_batch_reset clears it)");
  if (channels)
  {
    if (n > b->C)
      return fail(FMD_ERR_ARG, std::string(who) + ": more rows than the batch has channels");
    std::vector<unsigned> seen(channels, channels + n);
    std::sort(seen.begin(), seen.end());
    if (n && seen.back() >= b->C)
      return fail(FMD_ERR_ARG, std::string(who) + ": channel " + std::to_string(seen.back()) + " out of range");
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return fail(FMD_ERR_ARG, std::string(who) + ": a channel is listed twice");
  }
  else
    n = 0;
  fmd_batch::Selection& top = b->sel[kind];
  for (const Part& p : parts(b))
  {
    fmd_batch::Selection& sel = p.x->sel[kind];
    sel.ent.clear();
    for (unsigned i = 0; i < n; i++)
      if (channels[i] >= p.ch0 && channels[i] - p.ch0 < p.x->C)
        sel.ent.push_back(make_int2(int(channels[i] - p.ch0), int(i)));
    std::sort(sel.ent.begin(), sel.ent.end(), [](const int2& a, const int2& c) { return a.x < c.x; });
    sel.on = channels != nullptr;
    sel.n_total = n;
    sel.dirty = true;
  }
  top.on = channels != nullptr;
  top.n_total = n;
  if (channels)
    top.list.assign(channels, channels + n);
  else
    top.list.clear();
  return FMD_OK;
}

static int get_selection(fmd_batch* b, FormatKind kind, unsigned* out, unsigned cap, const char* who)
{
  if (!b || (cap && !out))
    return fail(FMD_ERR_ARG, std::string(who) + ": null argument");
  const fmd_batch::Selection& sel = b->sel[kind];
  const unsigned n = sel.on ? sel.n_total : b->C;
  for (unsigned i = 0; i < std::min(cap, n); i++)
    out[i] = sel.on ? sel.list[i] : i;
  return int(n);
}

int fmd_batch_select_audio(fmd_batch* b, const unsigned* channels, unsigned n)
{
  return select_rows(b, FMT_PCM, channels, n, "fmd_batch_select_audio");
}

int fmd_batch_select_mpx(fmd_batch* b, const unsigned* channels, unsigned n)
{
  return select_rows(b, FMT_MPX, channels, n, "fmd_batch_select_mpx");
}

int fmd_batch_get_audio_selection(fmd_batch* b, unsigned* out, unsigned cap)
{
  return get_selection(b, FMT_PCM, out, cap, "fmd_batch_get_audio_selection");
}

int fmd_batch_get_mpx_selection(fmd_batch* b, unsigned* out, unsigned cap)
{
  return get_selection(b, FMT_MPX, out, cap, "fmd_batch_get_mpx_selection");
}

int fmd_batch_select_feed(fmd_batch* b, const unsigned* channels, unsigned n)
{
  return select_rows(b, FMT_FEED, channels, n, "fmd_batch_select_feed");
}

int fmd_batch_get_feed_selection(fmd_batch* b, unsigned* out, unsigned cap)
{
  return get_selection(b, FMT_FEED, out, cap, "fmd_batch_get_feed_selection");
}

int fmd_batch_select_ciq(fmd_batch* b, const unsigned* channels, unsigned n)
{
  return select_rows(b, FMT_CIQ, channels, n, "fmd_batch_select_ciq");
}

int fmd_batch_get_ciq_selection(fmd_batch* b, unsigned* out, unsigned cap)
{
  return get_selection(b, FMT_CIQ, out, cap, "fmd_batch_get_ciq_selection");
}

/* fmd_batch_set_feed: a setup call.  It waits for the calls in flight (the scratch they may still write is freed or
 * replaced), then every batch with buffers takes the taps, a zeroed scratch and a frame count of 0. */
int fmd_batch_set_feed(fmd_batch* b, int divisor)
{
  if (divisor != 0 && divisor != 2 && divisor != 3)
    return fail(FMD_ERR_ARG, "fmd_batch_set_feed: the divisor must be 2 or 3, or 0 for no feed (any other is cut off "
                             "by the low-pass design's cap of 75 taps)");
  if (!b)
    return fail(FMD_ERR_ARG, "fmd_batch_set_feed: null batch");
  if (b->failed)
    return fail(FMD_ERR_ARG, "fmd_batch_set_feed: the batch has failed (fmd_batch_reset clears it)");
  std::vector<float> taps;
  if (divisor)
  {
    const float fs = float(b->params.sample_rate_pcm), fo = fs / float(divisor);
    taps = fmd::make_kaiser_lp(1.0f, 60.0f, 0.425f * fo, 0.575f * fo, fs);
    if (taps.size() < 2 || taps.size() > fmd::FEED_TAPS_MAX)
      return fail(FMD_ERR_ARG, "fmd_batch_set_feed: the low-pass design has no usable length at this rate");
  }
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  const unsigned T = unsigned(taps.size());
  for (const Part& p : parts(b))
  {
    fmd_batch* x = p.x;
    x->feed_div = 0; // (off until everything below is in place)
    x->feed_T = 0;
    x->feed_g = 0;
    x->feed_done.in_use = false;
    x->feed_x.release();
    x->feed_taps.release();
    if (!divisor)
      continue;
    if (x->feed_x.alloc(size_t(T - 1 + x->Amax) * x->CP) || x->feed_taps.alloc(T))
      return fail(FMD_ERR_DEVICE, "fmd_batch_set_feed: device allocation failed");
    HIPCHK(hipMemcpy(x->feed_taps.p, taps.data(), T * sizeof(float), hipMemcpyHostToDevice));
    if (!x->feed_done.e)
      HIPCHK(x->feed_done.create());
    x->feed_div = unsigned(divisor);
    x->feed_T = T;
  }
  HIPCHK(hipDeviceSynchronize());
  b->feed_div = unsigned(divisor);
  b->feed_T = T;
  b->feed_g = 0;
  b->feed_taps_h = taps;
  return FMD_OK;
}

int fmd_batch_get_feed(const fmd_batch* b)
{
  return b ? int(b->feed_div) : fail(FMD_ERR_ARG, "fmd_batch_get_feed: null batch");
}

double fmd_batch_feed_rate(const fmd_batch* b)
{
  return (b && b->feed_div) ? b->params.sample_rate_pcm / double(b->feed_div) : 0.0;
}

unsigned fmd_batch_max_feed_samples(const fmd_batch* b, unsigned samples)
{
  if (!b || !b->feed_div)
    return 0;
  // a call of A frames holds at most ceil(A / D) multiples of D
  return (fmd_batch_max_audio_floats(b, samples) / 2 + b->feed_div - 1) / b->feed_div;
}

int fmd_batch_get_feed_taps(const fmd_batch* b, float* out, unsigned cap)
{
  if (!b || (cap && !out))
    return fail(FMD_ERR_ARG, "fmd_batch_get_feed_taps: null argument");
  for (unsigned i = 0; i < std::min<size_t>(cap, b->feed_taps_h.size()); i++)
    out[i] = b->feed_taps_h[i];
  return int(b->feed_taps_h.size());
}

int fmd_batch_debug_ciq_in_skip_tile(fmd_batch* b, int on)
{
  if (!b)
    return fail(FMD_ERR_ARG, "null batch");
  set_all(b, &fmd_batch::dbg_ciq_in_skip, on != 0);
  return FMD_OK;
}

int fmd_batch_debug_feed_skip_roll(fmd_batch* b, int on)
{
  if (!b)
    return fail(FMD_ERR_ARG, "null batch");
  set_all(b, &fmd_batch::dbg_feed_skip_roll, on != 0);
  return FMD_OK;
}

int fmd_batch_retune_channels_to(fmd_batch* b, const unsigned* channels, const int* shifts, const unsigned* captures,
                                 unsigned n)
{
  if (!b || !channels || !shifts || !captures)
    return fail(FMD_ERR_ARG, "fmd_batch_retune_channels_to: null argument");
  if (!b->twin)
    return fail(FMD_ERR_STATE, "fmd_batch_retune_channels_to: retuning is not enabled (fmd_batch_enable_retune)");
  if (int rc = check_channel_list(b, channels, captures, n, "fmd_batch_retune_channels_to"))
    return rc;
  if (n == 0)
    return FMD_OK;
  if (int rc = ensure_map(b, "fmd_batch_retune_channels_to"))
    return rc;
  // the restart and the capture take effect at the same boundary, the next call's
  if (int rc = fmd_batch_retune_channels(b, channels, shifts, n))
    return rc;
  return fmd_batch_switch_captures(b, channels, captures, n);
}

int fmd_batch_set_concurrency(fmd_batch* b, int mode)
{
  if (!b || mode < 0 || mode > 2)
    return fail(FMD_ERR_ARG, "fmd_batch_set_concurrency: mode must be 0, 1 or 2");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  b->concurrency = mode;
  for (auto& sb : b->subs) // (their calls overlap inside one call of the shell; mode 1 is the shell's to keep)
    sb->concurrency = mode == 0 ? 0 : 2;
  return FMD_OK;
}

/* slots whose call is at least `lag` calls old and whose groups have not been taken out yet */
static bool slot_to_drain(const fmd_batch* b, int q, int lag)
{
  return slot_eligible(b, q, lag) && b->drained_call[q] != b->slot_call[q];
}

} // extern "C"

namespace
{

/* One drain of a queue family (fmd_batch::groups or ::blocks) of every part of b: the stream behind EV_RDS of the
 * slots that are `due`, one copy of the counts per part, ONE synchronisation, the records of the non-empty queues
 * back to back, at most one more synchronisation; then `done` for every slot visited and `take` for every part's
 * records.  Two synchronisations whatever the number of queues and of sub-batches; page-locked destinations: the
 * copies are DMA transfers, not staging kernels that would queue up behind the decoder's own.
 *
 * Where the two families differ, as they always did -- decided here and by the two callers, nowhere else:
 *  - which slots are due: the groups', whose newest call's groups were not taken yet (drained_call != slot_call,
 *    shared with the device export); the blocks', that a mode-2 call has used since the last drain (rb_dirty).
 *  - what overflow means: a queue keeps its first `cap` records in both; the groups' kernel has flagged the loss
 *    (FMD_WARN_RDS_LOST), the block collect adds the family's `over` to what it reports as lost.
 *  - how the staging grows: to the records found, and at least 2 C + 1024 groups / 4 C + 1024 block records.
 *  - the second synchronisation: sync_if_visited (the blocks) makes it whenever a slot was visited, else (the
 *    groups) only when records were copied. */
template <typename Q, typename Due, typename Done, typename Take>
int drain_queues(fmd_batch* b, Q fmd_batch::*family, hipStream_t stream, size_t grow_per_channel,
                        bool sync_if_visited, const char* who, Due due, Done done, Take take)
{
  const std::vector<Part> ps = parts(b);
  bool any = false, again = false;
  for (const Part& p : ps)
  {
    Q& q = p.x->*family;
    q.ntodo = 0;
    for (int slot = 0; slot < kSlots; slot++)
      if (due(p.x, slot)) // (not: never used / already drained / its call may still be appending)
      {
        HIPCHK(hipStreamWaitEvent(stream, p.x->cev[slot][fmd_batch::EV_RDS], 0));
        q.todo[q.ntodo++] = slot;
      }
    HIPCHK(q.fetch_counts(stream));
    any = any || q.ntodo > 0;
  }
  if (!any)
    return FMD_OK;
  HIPCHK(hipStreamSynchronize(stream));
  for (const Part& p : ps)
  {
    Q& q = p.x->*family;
    if (const int bad = q.fetch_records(grow_per_channel * p.x->C + 1024, stream))
      return fail(FMD_ERR_DEVICE, std::string(who) + (bad == -1 ? ": page-locked staging allocation failed"
                                                                : ": a copy out of the record queues failed"));
    again = again || (sync_if_visited ? q.ntodo > 0 : q.total > 0);
  }
  if (again)
    HIPCHK(hipStreamSynchronize(stream));
  for (const Part& p : ps)
  {
    Q& q = p.x->*family;
    for (int i = 0; i < q.ntodo; i++)
      done(p.x, q.todo[i]);
    take(p, q);
  }
  return FMD_OK;
}

} // namespace

extern "C" {

int fmd_batch_collect_rds_lagged(fmd_batch* b, fmd_rds_group* out, unsigned cap, int run_group_decoder,
                                 int lag, void* stream_)
{
  if (!b || lag < 0 || lag > 4)
    return fail(FMD_ERR_ARG, "fmd_batch_collect_rds: bad argument (lag must be 0..4)");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK(hipSetDevice(b->device));
  std::vector<fmd::RdsGroupRec> recs;
  if (int rc = drain_queues(
          b, &fmd_batch::groups, stream, 2, false, "fmd_batch_collect_rds",
          [lag](const fmd_batch* x, int q) { return slot_to_drain(x, q, lag); },
          [](fmd_batch* x, int q) { x->drained_call[q] = x->slot_call[q]; },
          [&recs](const Part& p, const auto& q) {
            const size_t at = recs.size();
            recs.insert(recs.end(), q.h_recs.p, q.h_recs.p + q.total);
            for (size_t i = at; i < recs.size(); i++)
              recs[i].channel += p.ch0;
          }))
    return rc;
  if (int rc = check_device_errors(b)) // the stream was synchronised above: covers the drained calls
    return rc;
  std::sort(recs.begin(), recs.end(), [](const fmd::RdsGroupRec& x, const fmd::RdsGroupRec& y) {
    if (x.call_index != y.call_index)
      return x.call_index < y.call_index;
    if (x.channel != y.channel)
      return x.channel < y.channel;
    return x.seq < y.seq;
  });
  unsigned k = 0;
  for (const auto& r : recs)
  {
    if (run_group_decoder && r.channel < b->C)
    {
      if (!b->shift_log.empty())
        gdec_follow_edits(b, r.channel, r.call_index);
      auto& g = b->gdec[r.channel];
      if (!g)
        g.reset(new fmd::GroupDecoder(&b->cb, b->user, r.channel));
      g->push(r.blocks);
    }
    if (out && k < cap)
    {
      out[k].channel = r.channel;
      out[k].call_index = r.call_index;
      for (int i = 0; i < 4; i++)
        out[k].blocks[i] = r.blocks[i];
      k++;
    }
  }
  return int(out ? k : recs.size());
}

int fmd_batch_collect_rds(fmd_batch* b, fmd_rds_group* out, unsigned cap, int run_group_decoder,
                          void* stream_)
{
  return fmd_batch_collect_rds_lagged(b, out, cap, run_group_decoder, 0, stream_);
}

/* The queues of one batch with buffers of its own, appended to the caller's record buffer at *cursor. */
static int export_queues(fmd_batch* b, int32_t* d_records, unsigned cap, unsigned channel_offset, int lag,
                         hipStream_t stream, unsigned* cursor)
{
  for (int q = 0; q < fmd_batch::NSLOT; q++)
  {
    if (!slot_to_drain(b, q, lag))
      continue; // also: already exported for its call -- one launch per call, not one per slot
    HIPCHK(hipStreamWaitEvent(stream, b->cev[q][fmd_batch::EV_RDS], 0));
    hipLaunchKernelGGL(fmd::k_rds_export, dim3(1), dim3(256), 0, stream, b->groups.queue[q].p, b->groups.count(q),
                       b->groups.cap, reinterpret_cast<int4*>(d_records), cap, cursor, channel_offset, b->st.err);
    HIPCHK(hipEventRecord(b->ev_drained[q], stream));
    b->drained_pending[q] = true;
    b->drained_call[q] = b->slot_call[q];
  }
  return FMD_OK;
}

int fmd_batch_export_rds_device(fmd_batch* b, int32_t* d_records, unsigned cap, unsigned channel_offset,
                                int lag, void* stream_)
{
  if (!b || !d_records || cap == 0 || lag < 0 || lag > 4)
    return fail(FMD_ERR_ARG, "fmd_batch_export_rds_device: bad argument (lag must be 0..4)");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemsetAsync(d_records, 0, size_t(cap) * 4 * sizeof(int32_t), stream));
  unsigned* const cursor = b->export_cursor.p + (b->export_seq++ % fmd_batch::kExportCursors);
  HIPCHK(hipMemsetAsync(cursor, 0, sizeof(unsigned), stream));
  for (const Part& p : parts(b))
    if (int rc = export_queues(p.x, d_records, cap, channel_offset + p.ch0, lag, stream, cursor))
      return rc;
  HIPCHK(hipGetLastError());
  if (int rc = check_device_errors(b))
    return rc;
  return take_lost_groups(b);
}

/* One output of a host call on its way through the device.  stage(): the device-side descriptor of host output h --
 * rows (one per channel, or the selection's) of at most cap elements in buf, grown on demand, at a stride that puts
 * every row on a 16-byte boundary; its count goes to n.  fetch(): the rows' n elements back into the caller's array,
 * laid out as that many rows (one row: packed). */
struct StagedOut
{
  Out dev{FMT_PCM};
  unsigned rows = 0, n = 0;
  int stage(DevBuf<float>& buf, const Out& h, const fmd_batch::Selection& sel, unsigned C, size_t cap)
  {
    rows = sel.on ? sel.n_total : C;
    const size_t round = 16 / h.esz() - 1;
    dev = h;
    dev.stride = (cap + round) & ~round;
    dev.out = &n;
    // (a selection of no rows stages one row nobody writes)
    const size_t floats = dev.stride * std::max(rows, 1u) * h.esz() / sizeof(float);
    if (floats > buf.n && buf.alloc(floats))
      return fail(FMD_ERR_DEVICE, "staging allocation failed");
    dev.p = buf.p;
    return FMD_OK;
  }
  int fetch(const Out& h) const
  {
    const size_t esz = h.esz();
    if (h.p && n && rows)
      HIPCHK(hipMemcpy2D(h.p, (rows > 1 ? h.stride : size_t(n)) * esz, dev.p, dev.stride * esz, size_t(n) * esz, rows,
                         hipMemcpyDeviceToHost));
    return FMD_OK;
  }
};

/* A host call that check_call_args has passed: staged in, one device call, staged out. */
static int process_host_impl(fmd_batch* b, const Call& c)
{
  HIPCHK(hipSetDevice(b->device));
  const unsigned C = b->C;
  // (channel IQ rows as input: the capture samples whose bounds hold for a call of this baseband length)
  const unsigned samples = c.ciq_in() ? std::min(c.samples, baseband_max(b)) * b->des.D : c.samples;
  // the outputs' staging -- audio; multiplex, feed and channel IQ where the call has them (the feed's rows one
  // element longer than fmd_batch_max_feed_samples)
  Call d = c;
  d.stream = nullptr;
  const size_t caps[FMT_KINDS] = {0, fmd_batch_max_audio_floats(b, samples), fmd_batch_max_mpx_samples(b, samples),
                                  size_t(fmd_batch_max_feed_samples(b, samples)) + 1,
                                  fmd_batch_max_mpx_samples(b, samples)};
  StagedOut so[FMT_KINDS];
  for (FormatKind k : kOutKinds)
    if (k == FMT_PCM || c.out(k).p)
    {
      if (int rc = so[k].stage(b->h_stage[k], c.out(k), b->sel[k], C, caps[k]))
        return rc;
      d.out(k) = so[k].dev;
    }
  const size_t esz = c.in_esz(); // bytes per input sample
  const unsigned n_in = c.samples;
  // device copy: one row per channel, rows padded to a whole pair of samples (channel IQ rows: to 16 bytes)
  const size_t dev_row = c.ciq_in() ? (size_t(n_in) * esz + 15) / 16 * 16 : (size_t(n_in) + 1) / 2 * 2 * esz;
  d.iq_stride = c.iq_stride ? dev_row / esz : 0;
  // input rows: one per capture of the map, per channel, per cpc channels, or one
  const unsigned streams = !c.iq_stride ? 1u : c.ciq_in() ? C : b->map_on ? b->n_cap : C / b->cpc;
  const size_t iq_floats = (dev_row * streams + 3) / 4;
  DevBuf<float>& h_iq = b->h_stage[FMT_IQ];
  if (iq_floats > h_iq.n && h_iq.alloc(iq_floats))
    return fail(FMD_ERR_DEVICE, "staging allocation failed");
  d.iq = h_iq.p;
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
  clk::time_point tp = clk::now();
  if (c.iq_stride)
    HIPCHK(hipMemcpy2D(h_iq.p, dev_row, c.iq, c.iq_stride * esz, size_t(n_in) * esz, streams,
                       hipMemcpyHostToDevice));
  else
    HIPCHK(hipMemcpy(h_iq.p, c.iq, size_t(n_in) * esz, hipMemcpyHostToDevice));
  b->host_ms[0] += ms_since(tp);
  tp = clk::now();
  int rc = process_any(b, d);
  if (rc != FMD_OK)
    return rc;
  const unsigned nf = so[FMT_PCM].n;
  if (so[FMT_PCM].rows > 1 && nf > c.audio.stride)
    return fail(FMD_ERR_ARG, "audio_channel_stride smaller than the audio produced");
  b->host_ms[1] += ms_since(tp);
  tp = clk::now();
  // Synchronous entry point in every concurrency mode: in mode 2 the null stream is not ordered after
  // the call -- order it behind the whole call before copying the audio out.
  rc = wait_impl(b, 0, nullptr, false); // the groups-lost flag is this call's to report, at its end
  if (rc < 0)
    return rc;
  for (FormatKind k : kOutKinds)
    if ((rc = so[k].fetch(c.out(k))))
      return rc;
  for (FormatKind k : {FMT_MPX, FMT_FEED, FMT_CIQ}) // (the audio's count: at the call's end)
    if (c.out(k).out)
      *c.out(k).out = so[k].n;
  b->host_ms[2] += ms_since(tp);
  tp = clk::now();
  rc = fmd_batch_collect_rds(b, nullptr, 0, 1, nullptr);
  if (rc < 0)
    return rc;
  b->host_ms[3] += ms_since(tp);
  b->host_calls++;
  if (c.audio.out)
    *c.audio.out = nf;
  return take_lost_groups(b); // FMD_OK, or FMD_WARN_RDS_LOST once: audio and state are intact
}

static int process_host_checked(const char* who, fmd_batch* b, Call& c)
{
  if (int rc = check_call_args(who, WAY_HOST, b, c))
    return rc;
  return process_host_impl(b, c);
}

int fmd_batch_process_host_pcm(fmd_batch* b, const void* iq, int iq_format, size_t iq_channel_stride,
                               unsigned samples, void* audio, int pcm_format, size_t audio_channel_stride,
                               unsigned* out_samples)
{
  Call c = make_call(iq, iq_format, iq_channel_stride, samples, audio, pcm_format, audio_channel_stride, out_samples);
  return process_host_checked("fmd_batch_process_host_pcm", b, c);
}

int fmd_batch_process_host_mpx(fmd_batch* b, const void* iq, int iq_format, size_t iq_channel_stride,
                               unsigned samples, void* audio, int pcm_format, size_t audio_channel_stride,
                               unsigned* out_samples, void* mpx, int mpx_format, size_t mpx_channel_stride,
                               unsigned* out_mpx_samples)
{
  Call c = make_call(iq, iq_format, iq_channel_stride, samples, audio, pcm_format, audio_channel_stride, out_samples);
  c.mpx = Out{FMT_MPX, mpx, mpx_format, mpx_channel_stride, out_mpx_samples};
  return process_host_checked("fmd_batch_process_host_mpx", b, c);
}

int fmd_batch_process_host_feed(fmd_batch* b, const void* iq, int iq_format, size_t iq_channel_stride,
                                unsigned samples, void* audio, int pcm_format, size_t audio_channel_stride,
                                unsigned* out_samples, void* mpx, int mpx_format, size_t mpx_channel_stride,
                                unsigned* out_mpx_samples, void* feed, int feed_format, size_t feed_channel_stride,
                                unsigned* out_feed_samples)
{
  Call c = make_call(iq, iq_format, iq_channel_stride, samples, audio, pcm_format, audio_channel_stride, out_samples);
  c.mpx = Out{FMT_MPX, mpx, mpx_format, mpx_channel_stride, out_mpx_samples};
  c.feed = Out{FMT_FEED, feed, feed_format, feed_channel_stride, out_feed_samples};
  return process_host_checked("fmd_batch_process_host_feed", b, c);
}

int fmd_batch_process_host_call(fmd_batch* b, const fmd_call* call)
{
  Call c;
  if (int rc = call_of_record("fmd_batch_process_host_call", call, c))
    return rc;
  return process_host_checked("fmd_batch_process_host_call", b, c);
}

int fmd_batch_process_host_fmt(fmd_batch* b, const void* iq, int format, size_t iq_channel_stride, unsigned samples,
                               float* audio, size_t audio_channel_stride, unsigned* out_floats)
{
  if (!format_ok(FMT_IQ, format))
    return fail(FMD_ERR_ARG, "fmd_batch_process_host_fmt: format must be one of FMD_IQ_F32, _U8, _S8, _S16 (0..3)");
  return fmd_batch_process_host_pcm(b, iq, format, iq_channel_stride, samples, audio, FMD_PCM_F32,
                                    audio_channel_stride, out_floats);
}

int fmd_batch_read_pcm_clipped(fmd_batch* b, unsigned first_channel, unsigned n, uint64_t* out)
{
  if (!b || !out)
    return fail(FMD_ERR_ARG, "fmd_batch_read_pcm_clipped: null argument");
  if (first_channel > b->C || n > b->C - first_channel)
    return fail(FMD_ERR_ARG, "fmd_batch_read_pcm_clipped: channels [" + std::to_string(first_channel) + ", " +
                                 std::to_string(size_t(first_channel) + n) + ") out of range (" +
                                 std::to_string(b->C) + " channels)");
  HIPCHK(hipSetDevice(b->device));
  // every call of this batch submitted so far, on whatever stream its audio tail runs: the null stream behind their
  // events, then the host behind the null stream (what the host-buffer call does before it copies the audio out)
  if (int rc = wait_impl(b, 0, nullptr, false); rc < 0)
    return rc;
  HIPCHK(hipStreamSynchronize(nullptr));
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counter's word");
  for (unsigned c = first_channel; c < first_channel + n;)
  { // run by run of channels with one owner (a shell: its sub-batches)
    unsigned lc = 0;
    const fmd_batch* ob = owner_of(b, c, &lc);
    const unsigned run = std::min(first_channel + n - c, ob->C - lc);
    HIPCHK(hipMemcpy(out + (c - first_channel), ob->pcm_clip.p + lc, size_t(run) * sizeof(uint64_t),
                     hipMemcpyDeviceToHost));
    c += run;
  }
  return FMD_OK;
}

/* ---- the block observation (fmd.h) ---- */
static_assert(sizeof(fmd_rds_block) == 24 && sizeof(fmd_rds_quality) == 32, "the records of fmd.h");
static_assert(sizeof(fmd_rds_quality) == fmd::RQ_N * sizeof(unsigned), "one word per counter, in the kernel's order");

int fmd_batch_set_rds_blocks(fmd_batch* b, int mode, unsigned queue_records)
{
  if (!b)
    return fail(FMD_ERR_ARG, "fmd_batch_set_rds_blocks: null batch");
  if (mode < FMD_RDS_BLOCKS_OFF || mode > FMD_RDS_BLOCKS_RECORD)
    return fail(FMD_ERR_ARG, "fmd_batch_set_rds_blocks: mode must be FMD_RDS_BLOCKS_OFF, _COUNT or _RECORD (0..2)");
  // (every part's queues hold the same number of records where the caller named one; else the first part's stands
  // for all in the refusal, as it always did)
  const unsigned have = first_part(b)->blocks.cap;
  if (queue_records && have && queue_records != have)
    return fail(FMD_ERR_ARG, "fmd_batch_set_rds_blocks: the block queues hold " + std::to_string(have) +
                                 " records since the first call that enabled mode 2; " +
                                 std::to_string(queue_records) + " refused");
  if (mode != FMD_RDS_BLOCKS_OFF)
  {
    HIPCHK(hipSetDevice(b->device));
    const std::vector<Part> ps = parts(b);
    for (const Part& p : ps)
      if (!p.x->rb_quality.p && p.x->rb_quality.alloc(size_t(fmd::RQ_N) * p.x->CP))
        return fail(FMD_ERR_DEVICE, "fmd_batch_set_rds_blocks: allocation of the counters failed");
    if (mode == FMD_RDS_BLOCKS_RECORD && !have)
      for (const Part& p : ps)
        if (p.x->blocks.alloc_counts() ||
            p.x->blocks.alloc_queues(queue_records ? queue_records : std::max(8192u, 4u * p.x->C)))
        { // nothing half-made stays: the batch is as before the call
          for (const Part& y : ps)
            y.x->blocks.release();
          return fail(FMD_ERR_DEVICE, "fmd_batch_set_rds_blocks: allocation of the block queues failed");
        }
  }
  set_all(b, &fmd_batch::rb_mode, mode);
  return FMD_OK;
}

int fmd_batch_get_rds_blocks(const fmd_batch* b)
{
  if (!b)
    return fail(FMD_ERR_ARG, "fmd_batch_get_rds_blocks: null batch");
  return b->rb_mode;
}

int fmd_batch_collect_rds_blocks(fmd_batch* b, fmd_rds_block* out, unsigned cap, int lag, void* stream_,
                                 unsigned* lost)
{
  if (!b || lag < 0 || lag > 4 || (!out && cap))
    return fail(FMD_ERR_ARG, "fmd_batch_collect_rds_blocks: bad argument (lag must be 0..4)");
  if (lost)
    *lost = 0;
  if (!first_part(b)->blocks.cap) // mode 2 was never enabled: no queue exists
    return 0;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK(hipSetDevice(b->device));
  std::vector<fmd_rds_block> recs;
  uint64_t dropped = 0;
  if (int rc = drain_queues(
          b, &fmd_batch::blocks, stream, 4, true, "fmd_batch_collect_rds_blocks",
          [lag](const fmd_batch* x, int q) { return x->rb_dirty[q] && slot_eligible(x, q, lag); },
          [](fmd_batch* x, int q) { x->rb_dirty[q] = false; },
          [&](const Part& p, const auto& q) {
            dropped += q.over; // a full queue kept its first `cap` records
            const size_t at = recs.size();
            recs.resize(at + q.total);
            for (size_t i = 0; i < q.total; i++)
            { // the device record's first 24 bytes are the caller's record
              std::memcpy(&recs[at + i], q.h_recs.p + 2 * i, sizeof(fmd_rds_block));
              recs[at + i].channel += p.ch0;
            }
          }))
    return rc;
  if (int rc = check_device_errors(b))
    return rc;
  std::sort(recs.begin(), recs.end(), [](const fmd_rds_block& x, const fmd_rds_block& y) {
    if (x.call_index != y.call_index)
      return x.call_index < y.call_index;
    if (x.channel != y.channel)
      return x.channel < y.channel;
    return int32_t(x.bit_index - y.bit_index) < 0; // (wrapping: the counter is modulo 2^32)
  });
  const size_t k = std::min<size_t>(recs.size(), cap);
  if (k)
    std::memcpy(out, recs.data(), k * sizeof(fmd_rds_block));
  dropped += recs.size() - k;
  if (lost)
    *lost = unsigned(std::min<uint64_t>(dropped, 0xFFFFFFFFu));
  return int(k);
}

int fmd_batch_read_rds_quality(fmd_batch* b, unsigned first_channel, unsigned n, fmd_rds_quality* out)
{
  if (!b || !out)
    return fail(FMD_ERR_ARG, "fmd_batch_read_rds_quality: null argument");
  if (first_channel > b->C || n > b->C - first_channel)
    return fail(FMD_ERR_ARG, "fmd_batch_read_rds_quality: channels [" + std::to_string(first_channel) + ", " +
                                 std::to_string(size_t(first_channel) + n) + ") out of range (" +
                                 std::to_string(b->C) + " channels)");
  std::memset(out, 0, size_t(n) * sizeof(fmd_rds_quality));
  unsigned probe = 0;
  if (!n || !owner_of(b, 0, &probe)->rb_quality.p) // never enabled: every counter is zero, and no device call
    return FMD_OK;
  HIPCHK(hipSetDevice(b->device));
  if (int rc = wait_impl(b, 0, nullptr, false); rc < 0)
    return rc;
  HIPCHK(hipStreamSynchronize(nullptr));
  std::vector<unsigned> rows;
  for (unsigned c = first_channel; c < first_channel + n;)
  { // run by run of channels with one owner (a shell: its sub-batches); the counters' rows, then transposed
    unsigned lc = 0;
    const fmd_batch* ob = owner_of(b, c, &lc);
    const unsigned run = std::min(first_channel + n - c, ob->C - lc);
    rows.resize(size_t(fmd::RQ_N) * run);
    HIPCHK(hipMemcpy2D(rows.data(), size_t(run) * sizeof(unsigned), ob->rb_quality.p + lc,
                       size_t(ob->CP) * sizeof(unsigned), size_t(run) * sizeof(unsigned), fmd::RQ_N,
                       hipMemcpyDeviceToHost));
    for (unsigned i = 0; i < run; i++)
    {
      uint32_t* w = reinterpret_cast<uint32_t*>(out + (c - first_channel) + i);
      for (int q = 0; q < fmd::RQ_N; q++)
        w[q] = rows[size_t(q) * run + i];
    }
    c += run;
  }
  return FMD_OK;
}

/* ---- the loudness meter (fmd.h) ---- */
static_assert(sizeof(fmd_loud_block) == 16 && sizeof(fmd_loud_block) == sizeof(float4), "the ring's record is fmd.h's");

int fmd_batch_set_loudness(fmd_batch* b, int mode, unsigned block_frames, unsigned ring_blocks)
{
  // (the arguments' own ranges first: they are refused whatever the batch)
  if (mode < FMD_LOUDNESS_OFF || mode > FMD_LOUDNESS_ON)
    return fail(FMD_ERR_ARG, "fmd_batch_set_loudness: mode must be FMD_LOUDNESS_OFF or FMD_LOUDNESS_ON (0..1)");
  if (block_frames && (block_frames < 16u || block_frames > (1u << 20)))
    return fail(FMD_ERR_ARG, "fmd_batch_set_loudness: block_frames must be 0 (100 ms) or 16 .. 1048576; " +
                                 std::to_string(block_frames) + " refused");
  if (ring_blocks && (ring_blocks < 8u || ring_blocks > 4096u))
    return fail(FMD_ERR_ARG, "fmd_batch_set_loudness: ring_blocks must be 0 (64) or 8 .. 4096; " +
                                 std::to_string(ring_blocks) + " refused");
  if (!b)
    return fail(FMD_ERR_ARG, "fmd_batch_set_loudness: null batch");
  if (b->loud_bf && block_frames && block_frames != b->loud_bf)
    return fail(FMD_ERR_ARG, "fmd_batch_set_loudness: a block is " + std::to_string(b->loud_bf) +
                                 " frames since the first call that turned the meter on; " +
                                 std::to_string(block_frames) + " refused");
  if (b->loud_bf && ring_blocks && ring_blocks != b->loud_ring)
    return fail(FMD_ERR_ARG, "fmd_batch_set_loudness: the ring holds " + std::to_string(b->loud_ring) +
                                 " blocks since the first call that turned the meter on; " +
                                 std::to_string(ring_blocks) + " refused");
  if (mode != FMD_LOUDNESS_OFF && !fmd::loud_tail_launch) // (never in the library: fmd_loud.hip)
    return fail(FMD_ERR_STATE, "fmd_batch_set_loudness: this build has no loudness kernels");
  if (mode != FMD_LOUDNESS_OFF && !b->loud_bf)
  {
    HIPCHK(hipSetDevice(b->device));
    const unsigned bf = block_frames ? block_frames : unsigned(std::lround(b->params.sample_rate_pcm / 10.0));
    const unsigned ring = ring_blocks ? ring_blocks : 64u;
    if (bf < 16u || bf > (1u << 20))
      return fail(FMD_ERR_ARG, "fmd_batch_set_loudness: 100 ms at this PCM rate is no block of 16 .. 1048576 frames");
    float coef[10];
    fmd::loud_design(b->params.sample_rate_pcm, coef);
    const std::vector<Part> ps = parts(b);
    for (const Part& p : ps)
      if (p.x->loud_state.alloc(size_t(fmd::LOUD_STATE_ROWS) * p.x->CP) ||
          p.x->loud_blocks.alloc(size_t(ring) * p.x->CP))
      { // nothing half-made stays: the batch is as before the call
        for (const Part& y : ps)
        {
          y.x->loud_state.release();
          y.x->loud_blocks.release();
        }
        return fail(FMD_ERR_DEVICE, "fmd_batch_set_loudness: allocation of the meter's state and ring failed");
      }
    set_all(b, &fmd_batch::loud_bf, bf);
    set_all(b, &fmd_batch::loud_ring, ring);
    std::copy(coef, coef + 10, b->loud_coef);
    for (auto& sb : b->subs)
      std::copy(coef, coef + 10, sb->loud_coef);
  }
  set_all(b, &fmd_batch::loud_mode, mode);
  return FMD_OK;
}

int fmd_batch_get_loudness(const fmd_batch* b)
{
  if (!b)
    return fail(FMD_ERR_ARG, "fmd_batch_get_loudness: null batch");
  return b->loud_mode;
}

unsigned fmd_batch_loudness_block_frames(const fmd_batch* b)
{
  if (!b)
    return 0;
  return b->loud_bf ? b->loud_bf : unsigned(std::lround(b->params.sample_rate_pcm / 10.0));
}

int fmd_batch_get_loudness_coeffs(const fmd_batch* b, float out[10])
{
  if (!b || !out)
    return fail(FMD_ERR_ARG, "fmd_batch_get_loudness_coeffs: null argument");
  fmd::loud_design(b->params.sample_rate_pcm, out);
  return FMD_OK;
}

int fmd_batch_debug_loud_skip_carry(fmd_batch* b, int on)
{
  if (!b)
    return fail(FMD_ERR_ARG, "null batch");
  set_all(b, &fmd_batch::dbg_loud_skip_carry, on != 0);
  return FMD_OK;
}

int fmd_batch_collect_loudness(fmd_batch* b, fmd_loud_block* out, unsigned cap_blocks, unsigned first_channel,
                               unsigned n_channels, int lag, void* stream_, uint64_t* first_block, unsigned* lost)
{
  if (!b || lag < 0 || lag > 4 || (!out && cap_blocks && n_channels))
    return fail(FMD_ERR_ARG, "fmd_batch_collect_loudness: bad argument (lag must be 0..4)");
  if (first_channel > b->C || n_channels > b->C - first_channel)
    return fail(FMD_ERR_ARG, "fmd_batch_collect_loudness: channels [" + std::to_string(first_channel) + ", " +
                                 std::to_string(size_t(first_channel) + n_channels) + ") out of range (" +
                                 std::to_string(b->C) + " channels)");
  if (lost)
    *lost = 0;
  if (first_block)
    *first_block = b->loud_taken;
  if (!b->loud_bf) // the meter was never on: no ring exists
    return 0;
  // the blocks the calls at least `lag` old have completed; of those, the ring still holds the ones that no call
  // submitted so far -- in flight or not -- has overwritten: the last loud_ring of all
  const fmd_batch* fp = first_part(b);
  const uint64_t avail = fp->loud_done[lag], total = fp->loud_done[0], ring = b->loud_ring;
  uint64_t start = b->loud_taken;
  const uint64_t oldest = std::min(avail, total > ring ? total - ring : uint64_t(0));
  if (oldest > start)
  {
    if (lost)
      *lost = unsigned(std::min<uint64_t>(oldest - start, 0xFFFFFFFFu));
    start = oldest;
  }
  const unsigned n = unsigned(std::min<uint64_t>(avail - start, cap_blocks));
  if (first_block)
    *first_block = start;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK(hipSetDevice(b->device));
  if (n && n_channels)
  {
    if (int rc = wait_impl(b, lag, stream_, false); rc < 0)
      return rc;
    HIPCHK(hipStreamSynchronize(stream));
    const size_t rec = sizeof(fmd_loud_block);
    for (unsigned c = first_channel; c < first_channel + n_channels;)
    { // run by run of channels with one owner (a shell: its sub-batches); the ring's rows in one or two pieces
      unsigned lc = 0;
      const fmd_batch* ob = owner_of(b, c, &lc);
      const unsigned run = std::min(first_channel + n_channels - c, ob->C - lc);
      for (unsigned k = 0; k < n;)
      {
        const unsigned row = unsigned((start + k) % ring);
        const unsigned rows = std::min(n - k, unsigned(ring) - row);
        HIPCHK(hipMemcpy2D(out + size_t(k) * n_channels + (c - first_channel), size_t(n_channels) * rec,
                           ob->loud_blocks.p + size_t(row) * ob->CP + lc, size_t(ob->CP) * rec, size_t(run) * rec,
                           rows, hipMemcpyDeviceToHost));
        k += rows;
      }
      c += run;
    }
  }
  else if (int rc = check_device_errors(b))
    return rc;
  b->loud_taken = start + n;
  return int(n);
}

double fmd_loudness_window(const fmd_loud_block* blk, unsigned n, unsigned block_frames)
{
  return fmd::loud_window(blk, n, block_frames);
}

double fmd_loudness_integrated(const fmd_loud_block* blk, unsigned n_blocks, unsigned block_frames)
{
  return fmd::loud_integrated(blk, n_blocks, block_frames);
}

int fmd_batch_process_host(fmd_batch* b, const float* iq, size_t iq_channel_stride, unsigned samples,
                           float* audio, size_t audio_channel_stride, unsigned* out_floats)
{
  return fmd_batch_process_host_fmt(b, iq, FMD_IQ_F32, iq_channel_stride, samples, audio, audio_channel_stride,
                                    out_floats);
}

int fmd_batch_process_host_u8(fmd_batch* b, const uint8_t* iq_u8, size_t iq_channel_stride,
                              unsigned samples, float* audio, size_t audio_channel_stride,
                              unsigned* out_floats)
{
  return fmd_batch_process_host_fmt(b, iq_u8, FMD_IQ_U8, iq_channel_stride, samples, audio, audio_channel_stride,
                                    out_floats);
}

/* The getters read the status snapshot the last kernel of every call leaves in host memory: no HIP
 * call, no stream operation, nothing of the batch's bookkeeping -- Kodi's status thread polls them
 * while the demux thread is inside ProcessStream (RadioReceiver.cpp:544-572 against :524). */
int fmd_batch_get_status(fmd_batch* b, unsigned channel, fmd_status* stt)
{
  if (!b || !stt || channel >= b->C)
    return fail(FMD_ERR_ARG, "fmd_batch_get_status: bad argument");
  unsigned w[fmd::HS_WORDS], lc = 0;
  const fmd_batch* ob = owner_of(b, channel, &lc); // (a shell: the sub-batch's snapshot)
  if (!host_status_read(ob, lc, w))
    return fail(FMD_ERR_DEVICE, "fmd_batch_get_status: the status snapshot is being written and never completes");
  auto f = [&](int i) {
    float v;
    memcpy(&v, &w[i], 4);
    return v;
  };
  stt->stereo_detected = int(w[fmd::HS_STEREO]);
  // FmDecode.h:146-150
  // the shift of the call the snapshot is of (a retuned channel: fmd_batch_retune_channels); a snapshot the host
  // wrote (create, reset) is of the newest call
  const uint32_t snap = (w[fmd::HS_SEQ_END] & 0x80000000u) ? __atomic_load_n(&b->call_index, __ATOMIC_RELAXED)
                                                            : w[fmd::HS_SEQ_END];
  const int shift = shift_at(b, channel, snap); // (the log is empty until the first retune, reset or import)
  const float tuned = float(-shift) * b->des.fs_if / float(int(b->des.table_size));
  stt->tuning_offset = tuned + f(fmd::HS_BB_MEAN) * b->des.freq_dev;
  stt->interface_level = f(fmd::HS_IF_LEVEL);
  stt->baseband_level = f(fmd::HS_BB_LEVEL);
  stt->pilot_level = 2 * f(fmd::HS_P_LEVEL); // FmDecode.h:75
  stt->rds_state = int(w[fmd::HS_R_STATE]);
  return FMD_OK;
}

int fmd_batch_get_audio_level(fmd_batch* b, unsigned channel, fmd_audio_level* out)
{
  if (!b || !out || channel >= b->C)
    return fail(FMD_ERR_ARG, "fmd_batch_get_audio_level: bad argument");
  unsigned w[fmd::HS_WORDS], lc = 0;
  const fmd_batch* ob = owner_of(b, channel, &lc); // (a shell: the sub-batch's snapshot)
  if (!host_status_read(ob, lc, w))
    return fail(FMD_ERR_DEVICE, "fmd_batch_get_audio_level: the status snapshot never completes");
  memcpy(&out->mean, &w[fmd::HS_AUDIO_MEAN], 4);
  memcpy(&out->rms, &w[fmd::HS_AUDIO_RMS], 4);
  memcpy(&out->level, &w[fmd::HS_AUDIO_LEVEL], 4);
  return FMD_OK;
}

int fmd_batch_status_call_index(fmd_batch* b, unsigned channel, uint32_t* call_index)
{
  if (!b || !call_index || channel >= b->C)
    return fail(FMD_ERR_ARG, "fmd_batch_status_call_index: bad argument");
  unsigned w[fmd::HS_WORDS], lc = 0;
  const fmd_batch* ob = owner_of(b, channel, &lc); // (a shell: the sub-batch's snapshot)
  if (!host_status_read(ob, lc, w))
    return fail(FMD_ERR_DEVICE, "fmd_batch_status_call_index: the status snapshot never completes");
  *call_index = (w[fmd::HS_SEQ_END] & 0x80000000u) ? 0u : w[fmd::HS_SEQ_END];
  return FMD_OK;
}

int fmd_batch_get_tap(fmd_batch* b, int tap, unsigned channel, float* out, unsigned cap_floats)
{
  if (!b || !out || channel >= b->C)
    return fail(FMD_ERR_ARG, "fmd_batch_get_tap: bad argument");
  if (is_shell(b))
  {
    unsigned lc = 0;
    fmd_batch* ob = owner_of(b, channel, &lc);
    return fmd_batch_get_tap(ob, tap, lc, out, cap_floats);
  }
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  const size_t CP = b->CP;
  const void* src = nullptr;
  size_t esize = 4, rows = 0, first_row = 0;
  const unsigned T_alp = unsigned(b->des.lpf_taps.size());
  switch (tap)
  {
    case FMD_TAP_DEMOD:
      if (size_t(2) * b->lastM > cap_floats)
        return fail(FMD_ERR_ARG, "tap buffer too small");
      HIPCHK(hipMemcpy(out, b->demod[b->call_index & 1u].p + size_t(channel) * b->Mstride, size_t(b->lastM) * 8,
                       hipMemcpyDeviceToHost));
      return int(b->lastM);
    /* windowed buffers were rolled at the end of the call: the block's rows are still in place
     * at [H, H+n) except the first H rows region, which now holds the tail -- read the data rows */
    case FMD_TAP_BASEBAND:
    case FMD_TAP_PILOT38:
    {
      rows = b->lastM;
      if (rows > cap_floats)
        return fail(FMD_ERR_ARG, "tap buffer too small");
      const char* s0 = reinterpret_cast<const char*>(b->brp(int(b->call_index & 1u))) +
                       (size_t(b->des.rs_order) * CP + channel) * 8 + (tap == FMD_TAP_PILOT38 ? 4 : 0);
      if (rows)
        HIPCHK(hipMemcpy2D(out, 4, s0, CP * 8, 4, rows, hipMemcpyDeviceToHost));
      return int(rows);
    }
    case FMD_TAP_MONO_RS:
    case FMD_TAP_STEREO_RS:
      src = reinterpret_cast<const float*>(b->rs[b->call_index & 1u].p) + (tap == FMD_TAP_MONO_RS ? 1 : 0);
      esize = 4;
      first_row = T_alp - 1;
      rows = b->lastA;
      {
        if (rows > cap_floats)
          return fail(FMD_ERR_ARG, "tap buffer too small");
        const char* s = reinterpret_cast<const char*>(src) + (first_row * CP + channel) * 8;
        HIPCHK(hipMemcpy2D(out, 4, s, CP * 8, 4, rows, hipMemcpyDeviceToHost));
        return int(rows);
      }
    case FMD_TAP_RDS_LPF:
      src = b->rlpf[b->call_index & 1u].p;
      esize = 8;
      rows = b->lastR;
      break;
    case FMD_TAP_RDS_PLL:
      src = b->rpll.p;
      first_row = b->des.rds_mf_taps.size() - 1;
      rows = b->lastR;
      break;
    case FMD_TAP_RDS_MF:
      src = b->rmf.p;
      rows = b->lastR;
      break;
    case FMD_TAP_RDS_SYNC:
      if (!b->write_taps)
        return fail(FMD_ERR_STATE, "RDS taps need fmd_batch_set_debug_taps(b, 1) before the call");
      src = b->tap_sync.p;
      rows = b->lastR;
      break;
    default:
      return fail(FMD_ERR_ARG, "unknown tap");
  }
  if (rows * (esize / 4) > cap_floats)
    return fail(FMD_ERR_ARG, "tap buffer too small");
  const char* s = reinterpret_cast<const char*>(src) + (first_row * CP + channel) * esize;
  if (rows)
    HIPCHK(hipMemcpy2D(out, esize, s, CP * esize, esize, rows, hipMemcpyDeviceToHost));
  return int(rows);
}

int fmd_batch_get_design(fmd_batch* b, int what, float* out, unsigned cap)
{
  if (!b || !out)
    return fail(FMD_ERR_ARG, "fmd_batch_get_design: bad argument");
  const fmd::Design& d = b->des;
  std::vector<float> v;
  switch (what)
  {
    case FMD_DESIGN_IF_TAPS:
      v = d.if_coeff;
      break;
    case FMD_DESIGN_RS_TAPS:
      v = d.rs_coeff;
      break;
    case FMD_DESIGN_AUDIO_LPF:
      v = d.lpf_taps;
      break;
    case FMD_DESIGN_RDS_LPF:
      v = d.rds_lpf_taps;
      break;
    case FMD_DESIGN_RDS_MF:
      v = d.rds_mf_taps;
      break;
    case FMD_DESIGN_LUT0:
      v = fmd::make_tuner_lut(d.table_size, b->shifts[0]);
      break;
    case FMD_DESIGN_SCALARS:
      v = {float(b->shifts[0]), d.demod_gain,  d.de_alpha,     d.pll_alpha,  d.pll_beta,
           d.nco_hl,            d.nco_ll,      d.p_minfreq,    d.p_maxfreq,  d.p_b0,
           d.p_a1,              d.p_a2,        d.p_lf_b0,      d.p_lf_b1,    d.p_freq0,
           float(d.p_lock_delay), float(d.rs_order), d.rs_step, d.rds_rate,  d.rds_nco_inc,
           d.rds_osc_cos,       d.rds_osc_sin, d.rds_pll_alpha, d.rds_pll_beta, d.rds_nco_hl,
           d.rds_nco_ll,        d.fs_bb,       float(d.rds_mf_taps.size()),
           d.notch.b0, d.notch.b1, d.notch.b2, d.notch.a1, d.notch.a2,
           d.bitsync.b0, d.bitsync.b1, d.bitsync.b2, d.bitsync.a1, d.bitsync.a2};
      break;
    default:
      return fail(FMD_ERR_ARG, "unknown design item");
  }
  for (size_t i = 0; i < v.size() && i < cap; i++)
    out[i] = v[i];
  return int(v.size());
}

int fmd_batch_set_debug_taps(fmd_batch* b, int enable)
{
  if (!b)
    return fail(FMD_ERR_ARG, "null batch");
  set_all(b, &fmd_batch::write_taps, enable != 0);
  return FMD_OK;
}

int fmd_batch_set_profiling(fmd_batch* b, int level)
{
  if (!b)
    return fail(FMD_ERR_ARG, "null batch");
  // Level 2 moves the next call onto the caller's stream with no event waits at all, and in
  // concurrency 2 that stream was never ordered behind the calls in flight: like set_concurrency,
  // a change of execution mode starts from an idle device.
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  set_all(b, &fmd_batch::profiling, level < 0 ? 0 : (level > 2 ? 2 : level));
  set_all(b, &fmd_batch::prof_calls, 0u); // restart the averaging window
  return FMD_OK;
}

int fmd_batch_get_stage_ms(fmd_batch* b, float* out, unsigned cap)
{
  if (!b || !out)
    return fail(FMD_ERR_ARG, "bad argument");
  if (is_shell(b))
  { // per call of the shell: the sub-batch calls' times added up (one launch of every stage per sub-batch)
    std::vector<float> sum(ST_COUNT, 0.0f), one(ST_COUNT);
    int calls = 0;
    for (auto& sb : b->subs)
    {
      const int n = fmd_batch_get_stage_ms(sb.get(), one.data(), ST_COUNT);
      if (n < 0)
        return n;
      calls = n;
      for (int i = 0; i < ST_COUNT; i++)
        sum[size_t(i)] = (one[size_t(i)] < 0 || sum[size_t(i)] < 0) ? -1.0f : sum[size_t(i)] + one[size_t(i)];
    }
    for (unsigned i = 0; i < cap && i < unsigned(ST_COUNT); i++)
      out[i] = sum[i];
    return calls;
  }
  if (!b->profiling || b->prof_calls == 0)
    return fail(FMD_ERR_STATE, "profiling not enabled or no call made since it was enabled");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  const int nst = b->profiling >= 2 ? ST_COUNT : 1;
  for (int i = 0; i < ST_COUNT; i++)
  {
    double sum = 0;
    if (i < nst)
      for (unsigned c = 0; c < b->prof_calls; c++)
      {
        float ms = 0;
        const Event* es = &b->ev[size_t(c) * (ST_COUNT + 1)];
        HIPCHK(hipEventElapsedTime(&ms, es[i], es[i + 1]));
        sum += ms;
      }
    if (unsigned(i) < cap)
      out[i] = i < nst ? float(sum / b->prof_calls) : -1.0f;
  }
  return int(b->prof_calls);
}

/* ---- single decoder = batch of one -------------------------------------------------------- */
struct fmd_decoder
{
  fmd_batch* b;
};

int fmd_create(const fmd_params* params, const fmd_callbacks* cb, void* user, fmd_decoder** out)
{
  if (!out)
    return fail(FMD_ERR_ARG, "null out");
  *out = nullptr;
  fmd_batch* b = nullptr;
  int dev = 0;
  (void)hipGetDevice(&dev);
  int rc = fmd_batch_create(params, 1, nullptr, dev, cb, user, &b);
  if (rc != FMD_OK)
    return rc;
  b->decoder_owned = true;
  *out = new fmd_decoder{b};
  return FMD_OK;
}

void fmd_destroy(fmd_decoder* d)
{
  if (!d)
    return;
  fmd_batch_destroy(d->b);
  delete d;
}

int fmd_reset(fmd_decoder* d)
{
  return d ? fmd_batch_reset(d->b) : fail(FMD_ERR_ARG, "null decoder");
}

/* fmd_process_stream_*: the formats, the decoder, then the host call of its batch; the audio's length on success */
static int process_stream_checked(const char* who, const char* host_who, fmd_decoder* d, Call& c)
{
  if (int rc = check_call_args(who, WAY_FORMATS, nullptr, c))
    return rc;
  if (!d)
    return fail(FMD_ERR_ARG, "null decoder");
  unsigned nf = 0;
  c.audio.out = &nf;
  const int rc = process_host_checked(host_who, d->b, c);
  return rc < 0 ? rc : int(nf); // (a groups-lost warning does not touch the audio: fmd_last_error has it)
}

int fmd_process_stream_pcm(fmd_decoder* d, const void* iq, int iq_format, unsigned samples, void* audio,
                           int pcm_format)
{
  Call c = make_call(iq, iq_format, 0, samples, audio, pcm_format, 0, nullptr);
  return process_stream_checked("fmd_process_stream_pcm", "fmd_batch_process_host_pcm", d, c);
}

int fmd_process_stream_mpx(fmd_decoder* d, const void* iq, int iq_format, unsigned samples, void* audio,
                           int pcm_format, void* mpx, int mpx_format, unsigned* mpx_samples)
{
  Call c = make_call(iq, iq_format, 0, samples, audio, pcm_format, 0, nullptr);
  c.mpx = Out{FMT_MPX, mpx, mpx_format, 0, mpx_samples};
  return process_stream_checked("fmd_process_stream_mpx", "fmd_batch_process_host_mpx", d, c);
}

int fmd_process_stream_feed(fmd_decoder* d, const void* iq, int iq_format, unsigned samples, void* audio,
                            int pcm_format, void* feed, int feed_format, unsigned* feed_samples)
{
  Call c = make_call(iq, iq_format, 0, samples, audio, pcm_format, 0, nullptr);
  c.feed = Out{FMT_FEED, feed, feed_format, 0, feed_samples};
  return process_stream_checked("fmd_process_stream_feed", "fmd_batch_process_host_feed", d, c);
}

int fmd_process_stream_call(fmd_decoder* d, const fmd_call* call)
{
  Call c;
  if (int rc = call_of_record("fmd_process_stream_call", call, c))
    return rc;
  // (host pointers of one channel: strides and stream are not looked at)
  c.iq_stride = c.audio.stride = c.mpx.stride = c.feed.stride = c.ciq.stride = 0;
  c.stream = nullptr;
  return process_stream_checked("fmd_process_stream_call", "fmd_batch_process_host_call", d, c);
}

int fmd_process_stream_fmt(fmd_decoder* d, const void* iq, int format, unsigned samples, float* audio)
{
  if (!format_ok(FMT_IQ, format))
    return fail(FMD_ERR_ARG, "fmd_process_stream_fmt: format must be one of FMD_IQ_F32, _U8, _S8, _S16 (0..3)");
  return fmd_process_stream_pcm(d, iq, format, samples, audio, FMD_PCM_F32);
}

int fmd_process_stream(fmd_decoder* d, const float* iq, unsigned samples, float* audio)
{
  return fmd_process_stream_fmt(d, iq, FMD_IQ_F32, samples, audio);
}

int fmd_process_stream_u8(fmd_decoder* d, const uint8_t* buf, unsigned samples, float* audio)
{
  return fmd_process_stream_fmt(d, buf, FMD_IQ_U8, samples, audio);
}

fmd_batch* fmd_decoder_batch(fmd_decoder* d)
{
  return d ? d->b : nullptr;
}

int fmd_get_status(fmd_decoder* d, fmd_status* st)
{
  return d ? fmd_batch_get_status(d->b, 0, st) : fail(FMD_ERR_ARG, "null decoder");
}

/* Test aid: the host build of fmd_ciq16_to_f32 (FMD_IN_CIQ_S16) on an array; no device is touched. */
int fmd_debug_ciq16_to_f32(const int16_t* in, unsigned n, float* out)
{
  if (!in || !out)
    return fail(FMD_ERR_ARG, "fmd_debug_ciq16_to_f32: null argument");
  for (unsigned i = 0; i < n; i++)
    out[i] = fmd_ciq16_to_f32(in[i]);
  return FMD_OK;
}

/* Test aid, see k_debug_math.  Host arrays in and out; b may be NULL for one-argument functions. */
int fmd_debug_math(int what, unsigned n, const float* a, const float* b, float* out0, float* out1)
{
  if (!a || !out0 || !out1 || n == 0)
    return fail(FMD_ERR_ARG, "fmd_debug_math: bad argument");
  fmd::Params p{};
  p.sample_rate_if = 2.4e6;
  p.sample_rate_pcm = 48000.0;
  p.bandwidth_pcm = 15000.0;
  p.downsample = 11;
  const fmd::Design d = fmd::make_design(p);
  DevBuf<float> da, db, d0, d1;
  DevBuf<double> tab, tab256;
  int bad = da.alloc(n) | db.alloc(n) | d0.alloc(n) | d1.alloc(n) | tab.alloc(d.sincos_tab.size()) |
            tab256.alloc(d.sincos_tab256.size());
  if (!bad)
  {
    bad |= hipMemcpy(da.p, a, size_t(n) * 4, hipMemcpyHostToDevice) != hipSuccess;
    if (b)
      bad |= hipMemcpy(db.p, b, size_t(n) * 4, hipMemcpyHostToDevice) != hipSuccess;
    bad |= hipMemcpy(tab.p, d.sincos_tab.data(), d.sincos_tab.size() * 8, hipMemcpyHostToDevice) !=
           hipSuccess;
    bad |= hipMemcpy(tab256.p, d.sincos_tab256.data(), d.sincos_tab256.size() * 8, hipMemcpyHostToDevice) !=
           hipSuccess;
  }
  if (!bad)
  {
    if (what == 8) // fmd_f32_to_s16: a kernel of its own
      hipLaunchKernelGGL(fmd::k_debug_pcm, dim3(std::min(4096u, (n + 63) / 64)), dim3(64), 0, nullptr, n, da.p, d0.p,
                         d1.p);
    else if (what == 9) // fmd_f32_to_mpx16
      hipLaunchKernelGGL(fmd::k_debug_mpx, dim3(std::min(4096u, (n + 63) / 64)), dim3(64), 0, nullptr, n, da.p, d0.p,
                         d1.p);
    else
      hipLaunchKernelGGL(fmd::k_debug_math, dim3(std::min(4096u, (n + 63) / 64)), dim3(64), 0, nullptr, what,
                         n, da.p, db.p, d0.p, d1.p, tab.p,
                         FmdSincosTab{d.sct_inv_h, d.sct_h_hi, d.sct_h_lo}, tab256.p);
    bad |= hipDeviceSynchronize() != hipSuccess;
    bad |= hipMemcpy(out0, d0.p, size_t(n) * 4, hipMemcpyDeviceToHost) != hipSuccess;
    bad |= hipMemcpy(out1, d1.p, size_t(n) * 4, hipMemcpyDeviceToHost) != hipSuccess;
  }
  return bad ? fail(FMD_ERR_DEVICE, "fmd_debug_math: device error") : FMD_OK;
}

int fmd_batch_debug_mpx_ms(fmd_batch* b, float* out, unsigned cap)
{
  if (!b || !out)
    return fail(FMD_ERR_ARG, "fmd_batch_debug_mpx_ms: null argument");
  if (is_shell(b)) // (the first sub-batch's calls)
    return fmd_batch_debug_mpx_ms(b->subs[0].get(), out, cap);
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  if (!b->dbg_mpx_timing)
  { // the first query: the calls from here on are timed
    for (int i = 0; i < fmd_batch::NSLOT; i++)
      for (int j = 0; j < 2; j++)
        HIPCHK(b->mpx_ev[i][j].create(hipEventDefault));
    b->dbg_mpx_timing = 1;
    return 0;
  }
  unsigned n = 0;
  for (int i = 0; i < fmd_batch::NSLOT && n < cap; i++)
  {
    float ms = 0.0f;
    if (b->mpx_ev[i][0].in_use && hipEventElapsedTime(&ms, b->mpx_ev[i][0], b->mpx_ev[i][1]) == hipSuccess)
      out[n++] = ms;
  }
  (void)hipGetLastError();
  return int(n);
}

int fmd_batch_debug_timeline(fmd_batch* b, float* out, unsigned cap_calls)
{
  if (!b || !out)
    return fail(FMD_ERR_ARG, "fmd_batch_debug_timeline: null argument");
  if (is_shell(b)) // (the first sub-batch's calls: every S-th of the common sequence)
    return fmd_batch_debug_timeline(b->subs[0].get(), out, cap_calls);
  if (b->profiling != 1 || b->prof_calls == 0 || !b->serial_exclusive || b->concurrency != 2)
    return 0;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  const unsigned n = std::min(cap_calls, b->prof_calls);
  hipEvent_t t0 = b->ev[0];
  for (unsigned c = 0; c < n; c++)
  {
    const Event* es = &b->ev[size_t(c) * (ST_COUNT + 1)];
    for (int i = 0; i < 10; i++)
    {
      float ms = -1.0f;
      if (hipEventElapsedTime(&ms, t0, es[i]) != hipSuccess)
        ms = -1.0f; // an event that was never recorded (the call's tail was not profiled)
      out[size_t(c) * 10 + i] = ms;
    }
  }
  (void)hipGetLastError();
  return int(n);
}

/* Which of the batch's internal streams share a hardware queue with `stream` (the caller's): bit i = internal
 * stream i (0 IF FIR, 1 serial stage, 2 heavy, 3 light RDS half, 4 light audio half / filters) had to wait for a wave
 * that kept `stream` busy; bit 8 + i = `stream` had to wait for internal stream i.  Drains the device. */
int fmd_batch_debug_stream_conflicts(fmd_batch* b, void* stream_)
{
  if (!b)
    return fail(FMD_ERR_ARG, "null batch");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  hipStream_t caller = static_cast<hipStream_t>(stream_);
  hipStream_t in[5] = {b->s_fir, b->s_ser, b->s_post, b->s_rds, b->s_lpf};
  const long long spin = 1200000; // ~0.5 ms
  int mask = 0;
  auto waits_behind = [&](hipStream_t busy, hipStream_t probe) {
    hipLaunchKernelGGL(fmd::k_probe_spin, dim3(1), dim3(64), 0, busy, spin, nullptr);
    const auto t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(fmd::k_probe_nop, dim3(1), dim3(64), 0, probe, nullptr);
    (void)hipStreamSynchronize(probe);
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    (void)hipStreamSynchronize(busy);
    return us >= 250.0;
  };
  for (int i = 0; i < 5; i++)
    if (in[i])
    {
      if (waits_behind(caller, in[i]))
        mask |= 1 << i;
      if (waits_behind(in[i], caller))
        mask |= 1 << (8 + i);
    }
  return mask;
}

int fmd_batch_debug_serial_probe(fmd_batch* b, long long* out, unsigned cap_workgroups)
{
  if (!b || !out)
    return fail(FMD_ERR_ARG, "fmd_batch_debug_serial_probe: null argument");
  if (is_shell(b))
    return fmd_batch_debug_serial_probe(b->subs[0].get(), out, cap_workgroups);
  if (!b->serial_probe.p)
    return 0;
  const unsigned wgs = std::min<unsigned>(cap_workgroups, unsigned(b->serial_probe.n / 3));
  // 8 launches x (CP / 64) slots, launch = call index mod 8 (the exclusive form uses every other slot's worth)
  if (hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(out, b->serial_probe.p, size_t(wgs) * 3 * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(FMD_ERR_DEVICE, "fmd_batch_debug_serial_probe: copy failed");
  return int(wgs);
}

} // extern "C"

#include "fmd_batch_state.inc.hpp" // fmd_batch_save_state / _load_state / _export_channels / _import_channels

/* ---- cRadioReceiver's stream side (csrc/fmd_receiver.hpp) ------------------------------------ */

fmd_batch* fmd::Receiver::fmd_decoder_batch(fmd_decoder* d)
{
  return d ? d->b : nullptr;
}

struct fmd_receiver
{
  fmd::Receiver r;
  fmd_receiver(const fmd_params& p, double tuner_freq, const char* name) : r(p, tuner_freq, name) {}
};

extern "C" {

int fmd_receiver_open(const fmd_params* params, double tuner_freq, const char* adapter_name,
                      fmd_receiver** out)
{
  if (!params || !out)
    return fail(FMD_ERR_ARG, "fmd_receiver_open: null argument");
  *out = nullptr;
  std::unique_ptr<fmd_receiver> r(new fmd_receiver(*params, tuner_freq, adapter_name));
  const int rc = r->r.Open(*params);
  if (rc != FMD_OK)
    return rc;
  *out = r.release();
  return FMD_OK;
}

void fmd_receiver_close(fmd_receiver* r)
{
  delete r;
}

int fmd_receiver_write_fmt(fmd_receiver* r, const void* buf, int format, unsigned samples)
{
  if (!format_ok(FMT_IQ, format))
    return fail(FMD_ERR_ARG, "fmd_receiver_write_fmt: format must be one of FMD_IQ_F32, _U8, _S8, _S16 (0..3)");
  if (!r || (!buf && samples))
    return fail(FMD_ERR_ARG, "fmd_receiver_write_fmt: null argument");
  if (!r->r.Write(buf, samples, format))
    return fail(FMD_ERR_DEVICE, "fmd_receiver_write_fmt: no page-locked memory for the block");
  return FMD_OK;
}

int fmd_receiver_write_iq(fmd_receiver* r, const float* iq, unsigned samples)
{
  if (!r || (!iq && samples))
    return fail(FMD_ERR_ARG, "fmd_receiver_write_iq: null argument");
  if (!r->r.Write(iq, samples, FMD_IQ_F32))
    return fail(FMD_ERR_DEVICE, "fmd_receiver_write_iq: no page-locked memory for the block");
  return FMD_OK;
}

int fmd_receiver_write_u8(fmd_receiver* r, const uint8_t* buf, unsigned samples)
{
  if (!r || (!buf && samples))
    return fail(FMD_ERR_ARG, "fmd_receiver_write_u8: null argument");
  if (!r->r.Write(buf, samples, FMD_IQ_U8))
    return fail(FMD_ERR_DEVICE, "fmd_receiver_write_u8: no page-locked memory for the block");
  return FMD_OK;
}

void fmd_receiver_end(fmd_receiver* r)
{
  if (r)
    r->r.End();
}

size_t fmd_receiver_queued_samples(fmd_receiver* r)
{
  return r ? r->r.QueuedSamples() : 0;
}

void fmd_receiver_set_stream_change(fmd_receiver* r)
{
  if (r)
    r->r.SetStreamChange();
}

int fmd_receiver_demux_read(fmd_receiver* r, fmd_demux_packet* pkt)
{
  if (!r || !pkt)
    return fail(FMD_ERR_ARG, "fmd_receiver_demux_read: null argument");
  return r->r.NextPacket(pkt);
}

int fmd_receiver_signal_status(fmd_receiver* r, float* interface_level_db, float* audio_level_db,
                               int* stereo)
{
  if (!r || !interface_level_db || !audio_level_db || !stereo)
    return fail(FMD_ERR_ARG, "fmd_receiver_signal_status: null argument");
  bool st = false;
  if (!r->r.Levels(*interface_level_db, *audio_level_db, st))
    return 0;
  *stereo = st ? 1 : 0;
  return 1;
}

int fmd_receiver_pvr_signal_status(fmd_receiver* r, fmd_pvr_signal_status* out)
{
  if (!r || !out)
    return fail(FMD_ERR_ARG, "fmd_receiver_pvr_signal_status: null argument");
  return r->r.PvrStatus(*out) ? 1 : 0;
}

fmd_decoder* fmd_receiver_decoder(fmd_receiver* r)
{
  return r ? r->r.Decoder() : nullptr;
}

/* ---- host-only pieces ----------------------------------------------------------------------- */
struct fmd_group_decoder
{
  fmd::GroupDecoder g;
  fmd_group_decoder(const fmd_callbacks* cb, void* user, unsigned ch) : g(cb, user, ch) {}
};

fmd_group_decoder* fmd_group_decoder_create(const fmd_callbacks* cb, void* user, unsigned channel)
{
  return new fmd_group_decoder(cb, user, channel);
}
void fmd_group_decoder_destroy(fmd_group_decoder* g)
{
  delete g;
}
void fmd_group_decoder_reset(fmd_group_decoder* g)
{
  if (g)
    g->g.reset();
}
void fmd_group_decoder_push(fmd_group_decoder* g, const uint16_t blocks[4])
{
  if (g)
    g->g.push(blocks);
}

static int copy_design(const std::vector<float>& v, float* out, unsigned cap)
{
  if (!out && cap)
    return -1;
  for (size_t i = 0; i < v.size() && i < cap; i++)
    out[i] = v[i];
  return int(v.size());
}

int fmd_design_lanczos(unsigned order, double cutoff, float* out, unsigned cap)
{
  if (order < 1)
    return -1;
  return copy_design(fmd::make_lanczos(order, cutoff), out, cap);
}

int fmd_design_lp_kaiser(float scale, float astop, float fpass, float fstop, float fs, float* out,
                         unsigned cap)
{
  return copy_design(fmd::make_kaiser_lp(scale, astop, fpass, fstop, fs), out, cap);
}

int fmd_design_biquad(int type, float f0, float q, float fs, float out[5])
{
  if (!out || type < 0 || type > 3)
    return -1;
  const fmd::Biquad b = fmd::make_biquad(fmd::BiquadType(type), f0, q, fs);
  out[0] = b.b0;
  out[1] = b.b1;
  out[2] = b.b2;
  out[3] = b.a1;
  out[4] = b.a2;
  return 5;
}

int fmd_design_tuner_lut(unsigned table_size, int freq_shift, float* out, unsigned cap)
{
  if (!table_size)
    return -1;
  return copy_design(fmd::make_tuner_lut(table_size, freq_shift), out, cap);
}

int fmd_uecp_stuff_frame(const uint8_t* frame, unsigned len, uint8_t* out, unsigned cap)
{
  if (!frame && len)
    return -1;
  unsigned k = 0;
  fmd::uecp_stuff(frame, len, [&](uint8_t v) {
    if (k < cap)
      out[k] = v;
    k++;
  });
  return k <= cap ? int(k) : -1;
}

} // extern "C"
