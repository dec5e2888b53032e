/*
 * fmd_batch_process.inc.hpp -- one call of a batch: the check in front of it (check_call, with the position plan of
 * fmd_call_plan.hpp: DownConvert.cpp:112-132, 203-232; FirFilter.cpp:346), the call while it is submitted (Submit),
 * the choice of kernel forms (decide_forms), one function per stage (stage_*, launch_light_*, launch_feed,
 * launch_ciq), the two schedules that put the stages on the batch's streams with the events that tie them
 * (submit_in_order, submit_overlapped behind the common submit_front), the position commit (commit_call) and the
 * entry that runs them (submit_call).
 * The record of the submission order -- which kernel goes to which stream, behind and in front of which event, in
 * every schedule -- is tests/test_call_trace_cpu.py with tests/golden/call_trace.txt: a change here that moves a
 * launch, a wait or a record shows up there as a readable diff, without a GPU.
 * Included by fmd_batch.hip behind fmd_batch_if.inc.hpp (one translation unit: it uses that file's fmd_batch
 * struct and helpers).
 */
namespace
{

/* The kernels' constant blocks, from the design (constructor maths: FmDecode.cpp:237-314, RDSProcess.cpp:60-90). */
fmd::DemodConsts demod_consts(const fmd::Design& d)
{
  fmd::DemodConsts k{};
  k.pll_alpha = d.pll_alpha;
  k.pll_beta = d.pll_beta;
  k.nco_hl = d.nco_hl;
  k.nco_ll = d.nco_ll;
  k.demod_gain = d.demod_gain;
  k.p_minfreq = d.p_minfreq;
  k.p_maxfreq = d.p_maxfreq;
  k.p_b0 = d.p_b0;
  k.p_a1 = d.p_a1;
  k.p_a2 = d.p_a2;
  k.p_lf_b0 = d.p_lf_b0;
  k.p_lf_b1 = d.p_lf_b1;
  k.p_minsignal = d.p_minsignal;
  k.p_lock_delay = d.p_lock_delay;
  k.osc_cos = d.rds_osc_cos;
  k.osc_sin = d.rds_osc_sin;
  return k;
}

fmd::RdsConsts rds_consts(const fmd::Design& d)
{
  fmd::RdsConsts k{};
  k.pll_alpha = d.rds_pll_alpha;
  k.pll_beta = d.rds_pll_beta;
  k.nco_hl = d.rds_nco_hl;
  k.nco_ll = d.rds_nco_ll;
  k.bs_b0 = d.bitsync.b0;
  k.bs_b1 = d.bitsync.b1;
  k.bs_b2 = d.bitsync.b2;
  k.bs_a1 = d.bitsync.a1;
  k.bs_a2 = d.bitsync.a2;
  k.mf_taps = int(d.rds_mf_taps.size());
  return k;
}

fmd::AudioConsts audio_consts(const fmd::Design& d)
{
  fmd::AudioConsts k{};
  k.de_alpha = d.de_alpha;
  k.n_b0 = d.notch.b0;
  k.n_b1 = d.notch.b1;
  k.n_b2 = d.notch.b2;
  k.n_a1 = d.notch.a1;
  k.n_a2 = d.notch.a2;
  return k;
}

/* The grid of a kernel that moves H history rows (k_roll, k_hb_pass, k_mix_tail): 256 channels per workgroup, at
 * most 64 rows of workgroups. */
inline dim3 roll_grid(unsigned CP, unsigned H)
{
  return dim3((CP + 255) / 256, std::max(1u, std::min(H, 64u)));
}

/* One of the ring-buffer filters of the post chain (cFirFilter::Process / ProcessTwo: RDS 75-tap low-pass and audio
 * 29-tap low-pass over float2, the RDS matched filter over float) on stream st; g0 = the ring phase at the call's
 * first sample; four: the unrolled kernel where the filter is long enough for it, with wave priority prio; origin:
 * the channels' ring origins where some were reset on their own (fmd_batch::org), else null. */
template <typename E>
void launch_ring(fmd_batch* b, hipStream_t st, const E* in, E* out, unsigned n, unsigned T, const float* taps,
                 unsigned g0, bool four, unsigned prio, const unsigned* origin)
{
  const unsigned C = b->C, CP = b->CP;
  const dim3 g4(CP / 64, (n + 4 * fmd::RG - 1) / (4 * fmd::RG)), gt(CP / 64, (n + fmd::RF_TI - 1) / fmd::RF_TI);
  const size_t lds = size_t(T - 1 + fmd::RF_TI) * 64 * sizeof(E);
  four = four && T >= unsigned(fmd::RG);
  if (origin && four)
    hipLaunchKernelGGL(fmd::k_ring_fir4_org<E>, g4, dim3(64, 4), 0, st, in, out, n, int(T), taps, g0, C, CP, 0u, prio,
                       origin);
  else if (origin)
    hipLaunchKernelGGL(fmd::k_ring_fir_org<E>, gt, dim3(64, 4), lds, st, in, out, n, int(T), taps, g0, C, CP, 0u,
                       origin);
  else if (four)
    hipLaunchKernelGGL(fmd::k_ring_fir4<E>, g4, dim3(64, 4), 0, st, in, out, n, int(T), taps, g0, C, CP, 0u, prio);
  else
    hipLaunchKernelGGL(fmd::k_ring_fir<E>, gt, dim3(64, 4), lds, st, in, out, n, int(T), taps, g0, C, CP, 0u);
}

/* History rolls of a chain whose stages all run in their normal regime are collected and done in one launch at the
 * chain's end (k_roll_set takes four) instead of one launch behind every stage. */
struct Rolls
{
  fmd::RollSet set{};
  unsigned n = 0, hmax = 1;
  void later(const float2* src, float2* dst, unsigned H, unsigned rows)
  {
    set.src[n] = src;
    set.dst[n] = dst;
    set.H[n] = H;
    set.n[n] = rows;
    n++;
    hmax = std::max(hmax, H);
  }
  void flush(unsigned CP, hipStream_t s)
  {
    if (n)
      hipLaunchKernelGGL(fmd::k_roll_set, dim3((CP + 255) / 256, std::min(hmax, 64u), n), dim3(256), 0, s, set, CP);
    n = 0;
    hmax = 1;
  }
};

/* A call while it is being submitted: the batch, the call and its plan, everything derived from the call's index,
 * the streams its parts go to, the kernel forms it takes (decide_forms), the first error of an event operation, the
 * profiling events and the collected rolls.  The stage functions below take it and a stream; the two schedules
 * (submit_in_order, submit_overlapped) are lists of waits, stages and signals over it.  The call's index and
 * everything derived from it live here until the call has been submitted (commit_call): a call that is refused
 * leaves the batch exactly as it was. */
struct Submit
{
  fmd_batch* const b;
  const Call& c;
  const fmd::CallPlan& pl;
  const fmd::Design& d = b->des;
  const unsigned C = b->C, CP = b->CP, M = pl.M, R = pl.R, A = pl.A;
  const unsigned T_lpf = unsigned(d.rds_lpf_taps.size()), T_mf = unsigned(d.rds_mf_taps.size());
  const unsigned T_alp = unsigned(d.lpf_taps.size()), Hbb = d.rs_order;
  const uint32_t ci = b->call_index + 1;
  const int q = int(ci & 1u);                // buffer parity: demod, br, mix
  const int es = int(ci % fmd_batch::NSLOT); // event set / RDS queue of this call
  const int sq = int(ci & 3u);               // this call's copy of the stereo flag (see ISlot)
  // call k-2 used the same buffers; its events say when they are free again.  pe1: the previous call's
  const bool have_prev2 = ci > 2;
  const Event* const ce = b->cev[es];
  const Event* const pe1 = b->cev[(ci + fmd_batch::NSLOT - 1) % fmd_batch::NSLOT];
  const Event* const pe2 = b->cev[(ci + fmd_batch::NSLOT - 2) % fmd_batch::NSLOT];
  const bool serial_mode = b->concurrency == 0 || b->profiling >= 2;
  /* "stage_mask" (fmd_batch_debug_set; results are WRONG with anything but 63): which parts of a call are
   * launched at all -- 1 IF stage, 2 serial stage, 4 half-band chain, 8 resampler, 16 / 32 the light part's RDS /
   * audio half.  Every event is still recorded, so the pipeline keeps its shape: tools/power_by_stage.py runs each
   * part alone at full rate beside a power sampler (joules per call and part). */
  const unsigned stage_mask = (!serial_mode && !b->split_post) ? unsigned(b->dbg_stage_mask) : 63u;
  const hipStream_t stream = static_cast<hipStream_t>(c.stream); // the caller's
  const hipStream_t sF = serial_mode ? stream : b->s_fir, sS = serial_mode ? stream : b->s_ser;
  const hipStream_t sP = serial_mode ? stream : b->s_post, sA = sP;
  const hipStream_t sR = (!serial_mode && b->split_post) ? b->s_rds : sP;
  const hipStream_t sL = serial_mode ? stream : b->s_rds; // the light part of an overlapped call
  // the ring origins of the RDS low-pass and matched filter, once a channel was reset on its own (the audio
  // low-pass is not reset: it never takes them)
  const unsigned* const rds_org = b->origins_live ? b->org.p : nullptr;
  hipError_t herr = hipSuccess; // the first failing event operation of the call (checked once, behind the launches)
  const Event* evset = nullptr; // the call's profiling events, or null

  // which forms the call takes (decide_forms)
  bool hb_all_normal = false;
  fmd_batch::HbfPlan* hbf_pl = nullptr; // the decimator as k_halfband_chain, or null: one launch per stage
  int hbf_kind = -1;                    // 0: 15 / 23 / 43 taps, 1: 15 / 19 / 35
  bool nomix = false;                   // the serial stage writes no mixed rows: the chain multiplies
  unsigned osc_slot = 0;
  float osc_re = b->osc_re, osc_im = b->osc_im; // committed with the positions, at the end
  bool ring = false, rs_planned = false;        // the resampler as k_resample_ring, else k_rs_table + k_resample
  unsigned rs_steps = 0;
  int layout = 0; // see the table in front of submit_overlapped
  Rolls rolls;

  // what differs between the schedules for the light part's two halves (launch_light_rds / launch_light_audio)
  int audio_after = -1;          // event of the call the audio half waits for on its stream (-1: stream order)
  bool status_after_rds = false; // the two halves are on different streams: the status record waits for EV_RDS
  hipEvent_t prev_aud = nullptr; // ... and the bit recovery for the previous call's status record
  hipEvent_t tl0 = nullptr, tl1 = nullptr; // profiling level 1: the audio tail's own start / stop

  Submit(fmd_batch* b_, const Call& c_, const fmd::CallPlan& pl_) : b(b_), c(c_), pl(pl_) {}
  Submit(const Submit&) = delete;

  void note(hipError_t e)
  {
    if (e != hipSuccess && herr == hipSuccess)
      herr = e;
  }
  void after(hipStream_t s, hipEvent_t e)
  {
    if (!serial_mode)
      note(hipStreamWaitEvent(s, e, 0));
  }
  void signal(hipEvent_t e, hipStream_t s)
  {
    if (!serial_mode)
      note(hipEventRecord(e, s));
  }
  // level 1, overlapped calls: events i, i + 1 take a kernel's own start and stop (fmd_batch_debug_timeline)
  hipEvent_t timed(int i) const { return evset && b->profiling == 1 && !serial_mode ? evset[i].e : nullptr; }
  // level 2: events between all stages (serial mode); events 0 and 1 are the FIR kernel's own start and stop
  // (launch_if_stage), also at level 1
  void mark(int i)
  {
    if (evset && b->profiling >= 2 && i > 1)
      note(hipEventRecord(evset[i], sF));
  }
  dim3 rgrid(unsigned H) const { return roll_grid(CP, H); }
};

/* A call appends its RDS groups to queue[es]; if the queue's previous contents were handed to an
 * asynchronous drain (fmd_batch_export_rds_device), stream s first waits for that drain. */
void queue_is_free(fmd_batch* b, int es, hipStream_t s)
{
  if (b->drained_pending[es])
  {
    if (hipStreamWaitEvent(s, b->ev_drained[es], 0) != hipSuccess)
      mark_failed(b, "hipStreamWaitEvent failed in front of an RDS queue");
    b->drained_pending[es] = false;
  }
}

/* The light part of a call's post chain, lane-per-channel kernels on CP / 64 workgroups, in two halves.
 * RDS half on stream s: (layout 2: the 75-tap low-pass behind the decimator's event,) cRDSRxSignalProcessor's
 * PLL, matched filter and bit recovery; records EV_RDS. */
void launch_light_rds(Submit& x, hipStream_t s)
{
  fmd_batch* const b = x.b;
  const fmd::Design& d = b->des;
  const unsigned C = b->C, CP = b->CP;
  const unsigned T_mf = x.T_mf, T_lpf = x.T_lpf;
  const dim3 rt(256);
  if (x.layout == 2)
  { // the RDS low-pass at the head of this stream, behind the decimator
    if (hipStreamWaitEvent(s, b->cev[x.es][fmd_batch::EV_DEC], 0) != hipSuccess)
      mark_failed(b, "hipStreamWaitEvent failed in front of the RDS low-pass of a call");
    launch_ring(b, s, b->rdsraw[x.q].p, b->rlpf[x.q].p, x.R, T_lpf, b->rds_lpf_taps.p, b->rds_lpf_g,
                b->dbg_ring4 != 0, 0u, x.rds_org);
    hipLaunchKernelGGL(fmd::k_roll<float2>, x.rgrid(T_lpf - 1), rt, 0, s, b->rdsraw[x.q].p, b->rdsraw[x.q ^ 1].p,
                       T_lpf - 1, x.R, CP);
    if (hipEventRecord(b->cev[x.es][fmd_batch::EV_RDSH], s) != hipSuccess)
      mark_failed(b, "hipEventRecord failed behind the RDS low-pass of a call");
  }
  queue_is_free(b, x.es, s);
  const fmd::RdsConsts k = rds_consts(d);
  const FmdSincosTab sct{d.sct_inv_h, d.sct_h_hi, d.sct_h_lo};
  hipLaunchKernelGGL(fmd::k_rds_pll, dim3((CP / 64 + fmd::RP_WAVES - 1) / fmd::RP_WAVES), dim3(64, fmd::RP_WAVES), 0,
                     s, b->rlpf[x.q].p, x.R, C, CP, k, b->st, b->rpll.p, T_mf - 1, b->sctab.p, sct);
  // the matched filter: between two lane-per-channel kernels, so at their wave priority; its origins: the second row
  launch_ring(b, s, b->rpll.p, b->rmf.p, x.R, T_mf, b->mf_taps2.p, b->mf_g, true, 3u,
              x.rds_org ? x.rds_org + CP : nullptr);
  hipLaunchKernelGGL(fmd::k_roll<float>, x.rgrid(T_mf - 1), rt, 0, s, b->rpll.p, b->rpll.p, T_mf - 1, x.R, CP);
  // Two light streams: the PREVIOUS call's status record (on the audio half's stream) copies the RDS state this
  // kernel is about to overwrite -- it goes first (its call's audio half ended a period ago: never a wait in practice)
  if (x.prev_aud && hipStreamWaitEvent(s, x.prev_aud, 0) != hipSuccess)
    mark_failed(b, "hipStreamWaitEvent failed in front of the bit recovery of a call");
  if (b->rb_mode == FMD_RDS_BLOCKS_OFF)
    hipLaunchKernelGGL(fmd::k_rds_bits, dim3(CP / 64), dim3(64, 1), 0, s, b->rmf.p, x.R, C, CP, k, b->st,
                       x.ci, b->groups.queue[x.es].p, b->groups.count(x.es), b->groups.cap, b->tap_sync.p, b->write_taps);
  else
  { // the observing forms (fmd_batch_set_rds_blocks): the same decoder, plus counters / block records
    fmd::RdsObs ob;
    ob.quality = b->rb_quality.p;
    const bool record = b->rb_mode == FMD_RDS_BLOCKS_RECORD;
    if (record)
    {
      ob.blocks = b->blocks.queue[x.es].p;
      ob.block_count = b->blocks.count(x.es);
      ob.block_cap = b->blocks.cap;
      b->rb_dirty[x.es] = true;
    }
    hipLaunchKernelGGL(record ? fmd::k_rds_bits_obs<true> : fmd::k_rds_bits_obs<false>, dim3(CP / 64), dim3(64, 1), 0,
                       s, b->rmf.p, x.R, C, CP, k, b->st, x.ci, b->groups.queue[x.es].p,
                       b->groups.count(x.es), b->groups.cap, b->tap_sync.p, b->write_taps, ob);
  }
  if (!x.serial_mode && hipEventRecord(b->cev[x.es][fmd_batch::EV_RDS], s) != hipSuccess)
    mark_failed(b, "hipEventRecord failed behind the RDS part of a call");
}

/* The row table of selection `sel` for a kernel about to be launched on stream st.  A
 * selection that changed since its current version was built takes a version nobody reads any more -- not the current
 * one, and the event behind its last reader has completed -- or a new one (only while the pool grows: as many
 * versions as calls are in flight, plus one), fills the version's own staging and uploads it on st, in front of the
 * reader.  A reader on another stream than the last one first waits for that one: the upload is in its order.
 * sel_read_done() behind the launch records the version's event.  Null: the batch has been marked failed. */
const int* sel_table(fmd_batch* b, fmd_batch::Selection& sel, bool mpx, hipStream_t st)
{
  if (sel.dirty || sel.cur < 0)
  {
    int v = -1;
    for (size_t i = 0; i < sel.pool.size() && v < 0; i++)
      if (int(i) != sel.cur && (!sel.pool[i]->read.in_use || hipEventQuery(sel.pool[i]->read) == hipSuccess))
        v = int(i);
    (void)hipGetLastError(); // (hipErrorNotReady is an answer, not an error)
    if (v < 0)
    {
      auto t = std::make_unique<fmd_batch::SelTable>();
      const size_t ints = mpx ? size_t(2) * b->C : size_t(b->CP);
      if (t->d.alloc(ints) || t->h.alloc(ints) || t->read.create() != hipSuccess)
      {
        mark_failed(b, "allocation of a selection's row table failed");
        return nullptr;
      }
      sel.pool.push_back(std::move(t));
      v = int(sel.pool.size()) - 1;
    }
    fmd_batch::SelTable& t = *sel.pool[v];
    size_t ints = 0;
    if (mpx)
    {
      for (const int2& e : sel.ent)
      {
        t.h.p[ints++] = e.x;
        t.h.p[ints++] = e.y;
      }
    }
    else
    {
      ints = b->CP;
      std::fill(t.h.p, t.h.p + ints, -1);
      for (const int2& e : sel.ent)
        t.h.p[e.x] = e.y;
    }
    if (ints && hipMemcpyAsync(t.d.p, t.h.p, ints * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess)
    {
      mark_failed(b, "the upload of a selection's row table failed");
      return nullptr;
    }
    t.stream = st;
    sel.cur = v;
    sel.dirty = false;
  }
  fmd_batch::SelTable& t = *sel.pool[sel.cur];
  if (t.stream != st && hipStreamWaitEvent(st, t.read, 0) != hipSuccess)
  {
    mark_failed(b, "hipStreamWaitEvent failed in front of a selection's row table");
    return nullptr;
  }
  return t.d.p;
}

void sel_read_done(fmd_batch* b, fmd_batch::Selection& sel, hipStream_t st)
{
  fmd_batch::SelTable& t = *sel.pool[sel.cur];
  if (t.read.record_use(st) != hipSuccess)
    mark_failed(b, "hipEventRecord failed behind a selection's row table");
  t.stream = st;
}

/* The rows of one output in the multiplex's form of selection (multiplex, feed, channel IQ) on stream s: with a
 * selection, selected(entries, their number) -- this batch's part of the list -- between the table's upload and the
 * event behind its reader, and nothing for an empty part or a failed batch; without, plain(). */
template <typename Selected, typename Plain>
void write_rows(fmd_batch* b, fmd_batch::Selection& sel, hipStream_t s, Selected selected, Plain plain)
{
  if (!sel.on)
    return plain();
  const unsigned n = unsigned(sel.ent.size());
  const int* tab = n ? sel_table(b, sel, true, s) : nullptr;
  if (!tab)
    return;
  selected(reinterpret_cast<const int2*>(tab), n);
  sel_read_done(b, sel, s);
}

/* The feed of a call behind the feed form of its audio tail, on the same stream: the decimating filter over history
 * and new rows into the caller's rows (k_feed_out, or the selected writer), then the roll that makes the last T - 1
 * rows the next feed call's history (the overlapping form for calls shorter than that), and the event behind it. */
void launch_feed(Submit& x, hipStream_t s)
{
  fmd_batch* const b = x.b;
  const unsigned C = b->C, CP = b->CP, T = b->feed_T, D = b->feed_div, n = x.pl.feed_n;
  const Out& f = x.c.feed;
  const unsigned tiles = (n + fmd::FEED_T - 1) / fmd::FEED_T;
  if (f.deliver && n)
    write_rows(
        b, b->sel[FMT_FEED], s,
        [&](const int2* ent, unsigned ns) { // (fmd_batch_select_feed): tiles of 64 entries
          const dim3 g((ns + 63) / 64, tiles);
          if (f.fmt == FMD_FEED_S16)
            hipLaunchKernelGGL(fmd::k_feed_out_sel<fmd::FeedS16>, g, dim3(256), 0, s, b->feed_x.p, b->feed_taps.p, T, D,
                               x.pl.feed_p0, n, ns, CP, ent, static_cast<int16_t*>(f.p), f.stride);
          else
            hipLaunchKernelGGL(fmd::k_feed_out_sel<fmd::FeedF32>, g, dim3(256), 0, s, b->feed_x.p, b->feed_taps.p, T, D,
                               x.pl.feed_p0, n, ns, CP, ent, static_cast<float*>(f.p), f.stride);
        },
        [&] {
          const dim3 g(CP / 64, tiles);
          if (f.fmt == FMD_FEED_S16)
            hipLaunchKernelGGL(fmd::k_feed_out<fmd::FeedS16>, g, dim3(256), 0, s, b->feed_x.p, b->feed_taps.p, T, D,
                               x.pl.feed_p0, n, C, CP, static_cast<int16_t*>(f.p), f.stride);
          else
            hipLaunchKernelGGL(fmd::k_feed_out<fmd::FeedF32>, g, dim3(256), 0, s, b->feed_x.p, b->feed_taps.p, T, D,
                               x.pl.feed_p0, n, C, CP, static_cast<float*>(f.p), f.stride);
        });
  if (!b->dbg_feed_skip_roll)
    hipLaunchKernelGGL(fmd::k_roll<float>, x.rgrid(T - 1), dim3(256), 0, s, b->feed_x.p, b->feed_x.p, T - 1, x.A, CP);
  if (b->feed_done.record_use(s) != hipSuccess)
    mark_failed(b, "hipEventRecord failed behind the feed of a call");
  b->feed_stream = s;
}

/* Audio half on stream s, behind event `audio_after` of the call where it has one: (layout 2: the 29-tap low-pass,)
 * de-emphasis, notch, L/R matrix, audio meter; then -- behind the RDS half -- the status record; records EV_AUD. */
void launch_light_audio(Submit& x, hipStream_t s)
{
  fmd_batch* const b = x.b;
  fmd_batch::Selection* const asel = b->sel[FMT_PCM].on ? &b->sel[FMT_PCM] : nullptr;
  const fmd::Design& d = b->des;
  const unsigned C = b->C, CP = b->CP;
  if (!x.serial_mode && x.audio_after >= 0 && hipStreamWaitEvent(s, b->cev[x.es][x.audio_after], 0) != hipSuccess)
    mark_failed(b, "hipStreamWaitEvent failed in front of the audio tail of a call");
  if (x.layout == 2)
  { // the audio low-pass in front of the tail that reads it
    launch_ring(b, s, b->rs[x.q].p, b->alp[x.q].p, x.A, x.T_alp, b->audio_taps.p, b->alpf_g, b->dbg_ring4 != 0, 0u,
                nullptr);
    hipLaunchKernelGGL(fmd::k_roll<float2>, x.rgrid(x.T_alp - 1), dim3(256), 0, s, b->rs[x.q].p, b->rs[x.q ^ 1].p,
                       x.T_alp - 1, x.A, CP);
  }
  const fmd::AudioConsts k = audio_consts(d);
  // (profiling level 1: x.tl0 / x.tl1 take the tail's own start and stop)
  // the call's output format is the tail's store policy (FMD_PCM_*): nothing in front of it sees the format
  // a selection (fmd_batch_select_audio): the selected forms and the call's row table; without, the kernels, the
  // arguments and the launches of a batch that never had one
  const int* rows = asel ? sel_table(b, *asel, false, s) : nullptr;
  // a call that asked for the feed (fmd_batch_set_feed): the feed forms, which also store every frame's mono mix into
  // the scratch rows behind the history.  The scratch is one buffer: this tail runs behind the last feed call's
  // k_feed_out and roll in stream order -- in every layout and concurrency mode the audio halves of a batch's calls
  // share one stream (the caller's, s_post, s_rds or s_lpf) until a setup call that drains the device moves them; a
  // stream that differs from the last feed call's all the same waits for the event behind that call's roll.
  float* const feed_rows = x.c.feed.p ? b->feed_x.p + size_t(b->feed_T - 1) * CP : nullptr;
  if (x.c.feed.p && b->feed_done.in_use && b->feed_stream != s && hipStreamWaitEvent(s, b->feed_done, 0) != hipSuccess)
    mark_failed(b, "hipStreamWaitEvent failed in front of the feed form of the audio tail");
  const bool s16 = x.c.audio.fmt == FMD_PCM_S16;
  auto tail = [&](auto kern, auto... more) { // (the forms differ in their last arguments)
    launch(kern, dim3(CP / 64), dim3(64, 1), 0, s, x.tl0, x.tl1, b->alp[x.q].p, x.A, C, CP, k, b->st, x.c.audio.p,
           x.c.audio.stride, unsigned(x.sq), x.ci, more...);
  };
  if (asel && !rows)
    ; // (the batch has failed: its state is void, the tail is left out)
  else if (b->loud_mode)
  { // a call submitted with the meter on (fmd_batch_set_loudness): the loudness forms (fmd_loud.hip), the meter's
    // record behind the form's own arguments.  State and ring are the tail's alone, in the stream order the channel state relies on.
    fmd::LoudArgs la;
    for (int sgi = 0; sgi < 2; sgi++)
    {
      la.b0[sgi] = b->loud_coef[5 * sgi];
      la.b1[sgi] = b->loud_coef[5 * sgi + 1];
      la.b2[sgi] = b->loud_coef[5 * sgi + 2];
      la.a1[sgi] = b->loud_coef[5 * sgi + 3];
      la.a2[sgi] = b->loud_coef[5 * sgi + 4];
    }
    la.state = b->loud_state.p;
    la.ring = b->loud_blocks.p;
    la.block_frames = b->loud_bf;
    la.left0 = b->loud_bf - unsigned(b->loud_g % b->loud_bf);
    la.ring_blocks = b->loud_ring;
    la.slot0 = unsigned((b->loud_g / b->loud_bf) % b->loud_ring);
    if (b->dbg_loud_skip_carry && // (mutation test: the block in progress is dropped at the call boundary)
        hipMemsetAsync(b->loud_state.p + size_t(fmd::LD_Z_L) * CP, 0, size_t(4) * CP * sizeof(float), s) != hipSuccess)
      mark_failed(b, "hipMemsetAsync failed in front of the loudness form of the audio tail");
    fmd::loud_tail_launch((s16 ? 1u : 0u) | (asel ? 2u : 0u) | (x.c.feed.p ? 4u : 0u), CP, s, x.tl0, x.tl1,
                          b->alp[x.q].p, x.A, C, k, b->st, x.c.audio.p, x.c.audio.stride, unsigned(x.sq), x.ci,
                          b->pcm_clip.p, rows, feed_rows, la);
  }
  else if (x.c.feed.p && asel)
    s16 ? tail(fmd::k_audio_tail_s16_sel_feed, b->pcm_clip.p, rows, feed_rows)
        : tail(fmd::k_audio_tail_sel_feed, rows, feed_rows);
  else if (x.c.feed.p)
    s16 ? tail(fmd::k_audio_tail_s16_feed, b->pcm_clip.p, feed_rows) : tail(fmd::k_audio_tail_feed, feed_rows);
  else if (asel)
    s16 ? tail(fmd::k_audio_tail_s16_sel, b->pcm_clip.p, rows) : tail(fmd::k_audio_tail_sel, rows);
  else
    s16 ? tail(fmd::k_audio_tail_s16, b->pcm_clip.p) : tail(fmd::k_audio_tail);
  if (rows)
    sel_read_done(b, *asel, s);
  if (x.c.feed.p)
    launch_feed(x, s);
  // the record's RDS state is the other half's (same stream: stream order)
  if (!x.serial_mode && x.status_after_rds && hipStreamWaitEvent(s, b->cev[x.es][fmd_batch::EV_RDS], 0) != hipSuccess)
    mark_failed(b, "hipStreamWaitEvent failed in front of the status record of a call");
  hipLaunchKernelGGL(fmd::k_status_publish, dim3((C + 255) / 256), dim3(256), 0, s, b->st, C, x.ci);
  if (!x.serial_mode && hipEventRecord(b->cev[x.es][fmd_batch::EV_AUD], s) != hipSuccess)
    mark_failed(b, "hipEventRecord failed behind the audio tail of a call");
}

/* The channel IQ of a call (the _call entry points): demod[q]'s rows, which the call's IF stage wrote, into the
 * caller's rows (k_ciq_out, or the selected writer), on the IF stage's own stream s right behind that stage (and its
 * level meter; EV_FIR is recorded in front: the serial stage does not wait for the writer and only reads the rows).
 * Stream order is the whole ordering argument: the rows' writer is in front on s, and their next writer -- the IF
 * stage of the next-but-one call -- is behind on s, in every stream layout, in serial mode (s is the caller's stream)
 * and with sub-batches and the silent twin (buffers of their own on the same s).  The call's EV_INDONE is recorded
 * behind the writer: fmd_batch_wait[_lagged] and the caller's stream wait for it with the audio and multiplex rows.
 * Measured against the other obvious place, the heavy stream beside the multiplex writer in front of EV_HEAVY
 * (DESIGN.md section 9.12): there a step took 0.06-0.08 ms longer.  A call without the rows launches nothing here. */
void launch_ciq(fmd_batch* b, const Out& o, int q, unsigned M, hipStream_t s)
{
  if (!o.p || !M)
    return;
  const bool s16 = o.fmt == FMD_CIQ_S16;
  const unsigned per = fmd::CIQ_G * (s16 ? fmd::CiqS16::PER : fmd::CiqF32::PER); // samples of a workgroup
  const unsigned tiles = (M + per - 1) / per;
  write_rows(
      b, b->sel[FMT_CIQ], s,
      [&](const int2* ent, unsigned n) { // (fmd_batch_select_ciq)
        if (s16)
          hipLaunchKernelGGL(fmd::k_ciq_out_sel<fmd::CiqS16>, dim3(n, tiles), dim3(fmd::CIQ_G), 0, s, b->demod[q].p,
                             b->Mstride, M, ent, static_cast<int16_t*>(o.p), o.stride);
        else
          hipLaunchKernelGGL(fmd::k_ciq_out_sel<fmd::CiqF32>, dim3(n, tiles), dim3(fmd::CIQ_G), 0, s, b->demod[q].p,
                             b->Mstride, M, ent, static_cast<float*>(o.p), o.stride);
      },
      [&] {
        if (s16)
          hipLaunchKernelGGL(fmd::k_ciq_out<fmd::CiqS16>, dim3(b->C, tiles), dim3(fmd::CIQ_G), 0, s, b->demod[q].p,
                             b->Mstride, M, static_cast<int16_t*>(o.p), o.stride);
        else
          hipLaunchKernelGGL(fmd::k_ciq_out<fmd::CiqF32>, dim3(b->C, tiles), dim3(fmd::CIQ_G), 0, s, b->demod[q].p,
                             b->Mstride, M, static_cast<float*>(o.p), o.stride);
      });
}

/* The position plan of call c from the positions of the batch (a shell: of its first sub-batch -- they all have the
 * same geometry and the same positions): of its samples, or, with channel IQ rows as input, of its baseband length. */
int plan_of_call(const fmd_batch* b, const Call& c, fmd::CallPlan& pl)
{
  const fmd_batch* x = b->subs.empty() ? b : b->subs[0].get();
  if (c.ciq_in())
    return fmd::plan_call_baseband(x->des, x->rs_pos, x->feed_g, b->feed_div, c.samples, pl);
  return fmd::plan_call(x->des, x->if_pos, x->rs_pos, x->feed_g, b->feed_div, c.samples, pl);
}

/* Everything that refuses a call, looked at before anything of it is submitted: a refused call leaves the batch as
 * it was, its pending channel edits included.  pl: the call's plan, from the positions of the batch (a shell: of its
 * first sub-batch -- they all have the same geometry and the same positions). */
int check_call(fmd_batch* b, const Call& c, fmd::CallPlan& pl)
{
  if (!b || !c.iq || (!c.audio.p && audio_rows_due(b)))
    return fail(FMD_ERR_ARG, "fmd_batch_process_device: null argument");
  if (c.ciq_in() && !fmd::ciq_in_launch) // (never in the library: fmd_k_ciq_in.hip.h)
    return fail(FMD_ERR_DEVICE, "the channel IQ input's kernels (fmd_ciq_in.o) are not linked into this program");
  if (c.ciq_in())
  { // (the plan's own refusals first: they are the sentences of an IQ call that would produce this length)
    if (c.samples > baseband_max(b))
      return fail(FMD_ERR_SIZE, "samples (the baseband length of a call with channel IQ rows as input) above the "
                                "batch's largest, fmd_batch_baseband_limits: " + std::to_string(baseband_max(b)));
    if (plan_of_call(b, c, pl) != FMD_OK)
      return fail(FMD_ERR_SIZE, pl.why);
    if (c.samples < baseband_min(b))
      return fail(FMD_ERR_SIZE, "samples (the baseband length of a call with channel IQ rows as input) must be within "
                                "fmd_batch_baseband_limits = [" + std::to_string(baseband_min(b)) + ", " +
                                    std::to_string(baseband_max(b)) + "]");
    // a lane loads 16 bytes of a row at a time: every row has to start on a 16-byte boundary
    if ((reinterpret_cast<uintptr_t>(c.iq) % 16) || (c.iq_stride * c.in_esz()) % 16)
      return fail(FMD_ERR_ARG, "with FMD_IN_CIQ_* the iq pointer must be 16-byte aligned and iq_channel_stride a "
                               "multiple of 2 (FMD_IN_CIQ_F32) / 4 (FMD_IN_CIQ_S16) complex samples");
  }
  else if (c.samples > FMD_MAX_BLOCK || c.samples < b->min_samples)
    return fail(FMD_ERR_SIZE, "samples must be within [fmd_batch_min_samples(), the largest block] = [" +
                                  std::to_string(b->min_samples) + ", 65536]");
  // a lane loads two IQ samples at a time: every channel's stream has to start on a pair boundary
  if (!c.ciq_in())
  {
    const size_t pair = 2 * format_esz(FMT_IQ, c.iq_fmt);
    if ((reinterpret_cast<uintptr_t>(c.iq) % pair) || ((c.iq_stride * (pair / 2)) % pair))
      return fail(FMD_ERR_ARG, "IQ pointer and channel stride must be multiples of two IQ samples");
  }
  HIPCHK(hipSetDevice(b->device));
  if (int rc = check_device_errors(b)) // a failed batch takes no more calls (fmd_batch_reset clears it)
    return rc;
  /* ---- position plan (batch-uniform, mirrors the reference's bookkeeping) ---- */
  if (plan_of_call(b, c, pl) != FMD_OK)
    return fail(FMD_ERR_SIZE, pl.why);
  if (pl.A > b->Amax || pl.M > b->Mmax)
    return fail(FMD_ERR_STATE, "internal: plan exceeds buffer geometry");
  // (the stride lies between rows: one row per channel, or the rows of the selection)
  if (size_t(2) * pl.A > c.audio.stride && (b->sel[FMT_PCM].on ? b->sel[FMT_PCM].n_total : b->C) > 1)
    return fail(FMD_ERR_ARG, "audio_channel_stride smaller than the audio produced");
  if (c.mpx.p && c.mpx.stride < pl.M)
    return fail(FMD_ERR_ARG, "mpx_channel_stride smaller than the call's baseband length");
  if (c.feed.p && !b->feed_div)
    return fail(FMD_ERR_STATE, "the feed is off (fmd_batch_set_feed)");
  if (c.feed.p && c.feed.stride < pl.feed_n)
    return fail(FMD_ERR_ARG, "feed_channel_stride smaller than the call's feed samples");
  if (c.ciq.p && c.ciq.stride < pl.M)
    return fail(FMD_ERR_ARG, "ciq.stride smaller than the call's baseband length");
  return FMD_OK;
}

/* Which forms the call takes: the RDS decimator's (the serial stage's follows from it), the resampler's, and the
 * stream layout of an overlapped call. */
void decide_forms(Submit& x)
{
  fmd_batch* const b = x.b;
  const fmd::Design& d = x.d;
  const unsigned groups = x.CP / 64;
  x.hb_all_normal = d.hb.size() <= 3;
  for (size_t s = 0; s < d.hb.size(); s++)
    x.hb_all_normal = x.hb_all_normal && x.pl.hb_mode[s] == fmd::HB_NORMAL && d.hb[s].len != 11 && !d.hb[s].cic;
  /* Large batches in the usual geometries: the three half-band stages as one stream, intermediate rows in
   * LDS (k_halfband_chain).  Everything else -- short calls with a stage outside its normal regime, the
   * 11-tap class, chains of another length, small batches -- keeps one launch per stage. */
  if (x.hb_all_normal && d.hb.size() == 3 && b->hbf_mode != 0 && (b->hbf_mode == 1 || groups >= 64))
  {
    const int h0 = (d.hb[0].len - 1) / 2, h1 = (d.hb[1].len - 1) / 2, h2 = (d.hb[2].len - 1) / 2;
    x.hbf_kind = (h0 == 7 && h1 == 11 && h2 == 21) ? 0 : (h0 == 7 && h1 == 9 && h2 == 17) ? 1 : -1;
    if (x.hbf_kind >= 0)
    {
      const unsigned ncu = unsigned(b->n_cus) - ((b->serial_exclusive && !x.serial_mode) ? (groups + 1) / 2 : 0u);
      const unsigned S = std::max(1u, std::min({8u, (2u * ncu + groups / 2u) / groups, x.R / 32u}));
      x.hbf_pl = hbf_plan(b, x.pl.hb_in[0], S);
    }
  }
  // ... and then the serial stage writes no mixed rows: the chain multiplies the baseband with the
  // oscillator's sequence itself (upload_oscillator)
  x.nomix = x.hbf_pl != nullptr && b->osc_on && b->dbg_nomix != 0 && b->osc_warm == 0;
  x.osc_slot = x.ci & 3u;
  /* Large batches stream the resampler's rows through an LDS ring (k_resample_ring: every row crosses the fabric
   * once per segment instead of ~6 times); small ones, short calls and geometries whose window does
   * not fit a CU's LDS keep the window-per-wave form, which has more workgroups to offer. */
  const unsigned per_step = unsigned(std::max(b->rsr_NW * b->rsr_R, 1));
  x.rs_steps = (x.A + per_step - 1) / per_step;
  x.ring = b->rsr_R != 0 && b->rsr_mode != 0 &&
           (b->rsr_mode == 1 || (groups >= 64 && x.rs_steps >= 24 && per_step >= 16));
  // (the table of layouts: in front of submit_overlapped)
  x.layout = (x.serial_mode || b->split_post) ? 0
             : b->dbg_lpf_late >= 0           ? b->dbg_lpf_late
             : d.if_order <= 512              ? 2
                                              : 0;
}

/* The call's profiling events (level 1: around the IF FIR and, overlapped, the timeline's kernels; level 2: between
 * all stages), created on first use; prof_calls advances with call_index. */
int take_profiling_events(Submit& x)
{
  fmd_batch* const b = x.b;
  if (!b->profiling || b->prof_calls >= kMaxProfCalls)
    return FMD_OK;
  const size_t need = size_t(b->prof_calls + 1) * (ST_COUNT + 1);
  while (b->ev.size() < need)
  {
    Event e;
    HIPCHK(e.create(hipEventDefault));
    b->ev.push_back(std::move(e));
  }
  x.evset = &b->ev[size_t(b->prof_calls) * (ST_COUNT + 1)];
  return FMD_OK;
}

/* The batch-wide RDS oscillator sequence of the call (fmd_batch::osc_on): computed here, once per batch and call,
 * and copied over on the IF stream: long before anything needs it. */
void upload_oscillator(Submit& x)
{
  fmd_batch* const b = x.b;
  if (!b->osc_on)
    return;
  // the staging slot was last read by the copy of the call 8 calls ago: complete unless the caller has
  // submitted eight calls without ever waiting
  x.note(b->osc_ev[x.es].sync_if_in_use());
  fmd::HbOsc* h = b->h_osc.p + size_t(x.es) * b->h_osc_stride;
  const fmd::HbOsc* hp = b->h_osc.p + size_t((x.ci + fmd_batch::NSLOT - 1) % fmd_batch::NSLOT) * b->h_osc_stride;
  std::memcpy(h, hp + b->lastM, fmd_batch::kOscH * sizeof(fmd::HbOsc)); // the previous call's last entries
  const float oc = x.d.rds_osc_cos, os = x.d.rds_osc_sin;
  fmd::HbOsc* o = h + fmd_batch::kOscH;
  // the two products of the chain's complex multiplication that are the same for every channel (HbOsc::z): IEEE
  // multiplications by zero like the device's (a signed zero each; volatile: never folded)
  const volatile float zero = 0.0f;
  float osc_re = x.osc_re, osc_im = x.osc_im;
  for (unsigned t = 0; t < x.M; t++)
  { // the statements of k_demod_serial's MIX form (this file is compiled with -ffp-contract=off too)
    const float u = osc_re * oc - osc_im * os;
    const float v = osc_im * oc + osc_re * os;
    const float gn = float(1.95 - double(osc_re * osc_re + osc_im * osc_im));
    osc_re = gn * u;
    osc_im = gn * v;
    o[t].xy = make_float2(u, v);
    o[t].z = make_float2(-(zero * v), zero * u);
  }
  x.osc_re = osc_re;
  x.osc_im = osc_im;
  x.note(hipMemcpyAsync(b->osc_tab[x.osc_slot].p, h, (fmd_batch::kOscH + x.M) * sizeof(fmd::HbOsc),
                        hipMemcpyHostToDevice, x.sF));
  x.note(b->osc_ev[x.es].record_use(x.sF));
}

/* A capture map that changed since the last call (switches, retunes to a capture, a new map): the walk table goes
 * to the device on the IF stage's stream, behind every earlier call's IF stage (the level meter included) and in
 * front of this one's.  No other wait: a call with switches overlaps the calls before it like any other call. */
void upload_walk(Submit& x)
{
  fmd_batch* const b = x.b;
  if (!b->map_on || !b->map_dirty)
    return;
  x.note(b->walk_ev[x.es].sync_if_in_use()); // the copy of 8 calls ago
  uint2* h = b->h_walk.p + size_t(x.es) * x.C;
  build_walk(b, h);
  x.note(hipMemcpyAsync(b->d_walk.p, h, x.C * sizeof(uint2), hipMemcpyHostToDevice, x.sF));
  x.note(b->walk_ev[x.es].record_use(x.sF));
  b->map_dirty = false;
}

/* K1: tuner + IF decimating FIR and the level meter on the IF stream; EV_FIR right behind the FIR kernel (the serial
 * stage waits for nothing else). */
int stage_if(Submit& x)
{
  const std::function<void(int)> markfn = [&x](int i) {
    x.mark(i);
    if (i == 1)
      x.signal(x.ce[fmd_batch::EV_FIR], x.sF);
  };
  if (!(x.stage_mask & 1u))
  { // (energy experiment: this call leaves the IF stage out -- see "stage_mask")
    markfn(1);
    return FMD_OK;
  }
  if (x.c.ciq_in())
  { // channel IQ rows as input: the copy into demod[q] is the whole stage -- no tuner, no FIR, no level meter, and the
    // stage's carried state (history, tuner phase, decimator phase) is not touched (commit_call).  The profiling
    // events of the FIR kernel take the copy's start and stop: the stage-time getter reports it in the IF stage's slot.
    const bool s16 = x.c.iq_fmt == FMD_IN_CIQ_S16;
    const unsigned per = fmd::CIQ_G * (s16 ? fmd::InCiqS16::PER : fmd::InCiqF32::PER); // samples of a workgroup
    // (fmd_batch_debug_ciq_in_skip_tile, a mutation test's: every row's last tile is left out)
    const unsigned tiles = (x.M + per - 1) / per - (x.b->dbg_ciq_in_skip ? 1u : 0u);
    const hipEvent_t t0 = x.evset ? x.evset[0].e : nullptr, t1 = x.evset ? x.evset[1].e : nullptr;
    markfn(0);
    if (tiles) // (the kernels' own object: fmd_ciq_in.hip)
      fmd::ciq_in_launch(s16, x.C, tiles, x.sF, t0, t1, x.c.iq, x.c.iq_stride, x.M, x.b->demod[x.q].p, x.b->Mstride);
    markfn(1);
    return FMD_OK;
  }
  auto go = [&](auto in) { // launch_if_stage<IN> of the call's format
    return launch_if_stage<decltype(in)>(x.b, x.c.iq, x.c.iq_stride, x.c.samples, x.b->if_pos, x.M, x.q, x.sF, markfn,
                                         x.evset ? x.evset[0].e : nullptr, x.evset ? x.evset[1].e : nullptr);
  };
  switch (IqFormat(x.c.iq_fmt))
  {
  case IQ_U8:
    return go(fmd::InU8{});
  case IQ_S8:
    return go(fmd::InS8{});
  case IQ_S16:
    return go(fmd::InS16{});
  default:
    return go(fmd::InF32{});
  }
}

/* K2: the baseband-rate recurrences on the serial stream. */
void stage_serial(Submit& x)
{
  fmd_batch* const b = x.b;
  const fmd::Design& d = x.d;
  if (!(x.stage_mask & 2u)) // (the energy experiment: no serial stage in this call)
    return;
  const fmd::DemodConsts k = demod_consts(d);
  // From 1024 channels on the stage owns whole CUs: two channel groups per workgroup, one role wave per SIMD of a
  // CU (k_demod_serial<2, ..>; at most 64 CUs: larger batches are sub-batches); smaller batches share their CUs.
  const unsigned groups = x.CP / 64;
  const FmdSincosTab sct{d.sct_inv_h, d.sct_h_hi, d.sct_h_lo};
  const unsigned Hmix = unsigned(d.hb[0].len - 1);
  /* Two groups per workgroup = one role wave on each SIMD of a CU, 64 CUs for 8192 channels.  The waves do not
   * claim their SIMD's whole register file (round 3: the bandwidth kernels' waves that fit beside the stage gain
   * more than it loses, +1-2 % whole path); "serial_claim" = 1 of fmd_batch_debug_set brings the claim back. */
  const bool serial_claim = b->dbg_serial_claim != 0;
  auto kser2 = x.nomix ? (serial_claim ? &fmd::k_demod_serial<2, true, false> : &fmd::k_demod_serial<2, false, false>)
                       : (serial_claim ? &fmd::k_demod_serial<2, true, true> : &fmd::k_demod_serial<2, false, true>);
  auto kser1 = x.nomix ? &fmd::k_demod_serial<1, false, false> : &fmd::k_demod_serial<1, false, true>;
  const bool whole_cu = b->serial_exclusive && !x.serial_mode;
  const hipEvent_t t0 = whole_cu ? x.timed(2) : nullptr, t1 = whole_cu ? x.timed(3) : nullptr;
  // (the timed launch takes no serial probe)
  long long* probe = b->serial_probe.p && !t0 ? b->serial_probe.p + size_t(x.ci % 8) * 3 * groups : nullptr;
  launch(whole_cu ? kser2 : kser1, dim3(whole_cu ? (groups + 1) / 2 : groups), dim3(whole_cu ? 256 : 128), 0, x.sS, t0,
         t1, b->demod[x.q].p, b->Mstride, x.M, x.C, x.CP, k, b->st, b->brp(x.q), x.Hbb, b->mix[x.q].p, Hmix,
         b->sctab256.p, sct, unsigned(x.sq), probe, x.osc_re, x.osc_im);
}

/* With overlapped calls the next call's serial stage and this call's post chain become runnable the moment this
 * call's serial stage ends.  The whole-CU serial stage needs EMPTY CUs; when the half-band kernel is dispatched first
 * it fills every CU and the serial stage starts only once those workgroups have drained (136 us late, every call).
 * So the post chain starts behind a single wave that idles for a few microseconds: the serial stage is dispatched
 * first (30-50 us after its predecessor, period 2.50 -> 2.42 ms). */
void stage_post_delay(Submit& x, hipStream_t s)
{
  constexpr unsigned kPostDelayUs = 20;
  if (x.b->serial_exclusive && !x.serial_mode && x.b->concurrency == 2)
    hipLaunchKernelGGL(fmd::k_delay, dim3(1), dim3(64), 0, s, kPostDelayUs * 100u);
}

/* The RDS decimator as one kernel (k_halfband_chain, x.hbf_pl); its rolls are collected. */
void stage_decimator_chain(Submit& x, hipStream_t s)
{
  fmd_batch* const b = x.b;
  const fmd::Design& d = x.d;
  const unsigned L0H = unsigned(d.hb[0].len - 1);
  // stage 0's input rows and, without mixed rows, the oscillator entries that go with them: both
  // indexed by the stage's input row (0 = the first of its L0H history rows)
  const float2* in0 = x.nomix ? (const float2*)(b->brp(x.q) + size_t(x.Hbb - L0H) * x.CP) : (const float2*)b->mix[x.q].p;
  const fmd::HbOsc* osc = x.nomix ? b->osc_tab[x.osc_slot].p + (fmd_batch::kOscH - L0H) : nullptr;
  auto kern = x.hbf_kind == 0
                  ? (x.nomix ? &fmd::k_halfband_chain<7, 11, 21, true> : &fmd::k_halfband_chain<7, 11, 21, false>)
                  : (x.nomix ? &fmd::k_halfband_chain<7, 9, 17, true> : &fmd::k_halfband_chain<7, 9, 17, false>);
  launch(kern, dim3(x.CP / 64, x.hbf_pl->S), dim3(64, 4), 0, s, x.timed(6), x.timed(7), in0, b->hbbuf[0].p,
         b->hbbuf[1].p, b->rdsraw[x.q].p + size_t(x.T_lpf - 1) * x.CP, b->hb_taps, (const fmd::HbStep*)x.hbf_pl->steps.p,
         (const int*)x.hbf_pl->seg_first.p, x.C, x.CP, osc, 0u);
  if (!x.nomix) // (without mixed rows: stage_mix_tail, where the schedule puts it)
    x.rolls.later(b->mix[x.q].p, b->mix[x.q ^ 1].p, L0H, x.pl.hb_in[0]);
  x.rolls.later(b->hbf_tail1.p, b->hbbuf[0].p, unsigned(d.hb[1].len - 1), 0u);
  x.rolls.later(b->hbf_tail2.p, b->hbbuf[1].p, unsigned(d.hb[2].len - 1), 0u);
}

/* Behind a chain without mixed rows: the next call's stage-0 history, should it take a launch per stage (it reads
 * mixed rows). */
void stage_mix_tail(Submit& x, hipStream_t s)
{
  fmd_batch* const b = x.b;
  const unsigned L0H = unsigned(x.d.hb[0].len - 1), n0 = x.pl.hb_in[0];
  hipLaunchKernelGGL(fmd::k_mix_tail, x.rgrid(L0H), dim3(256), 0, s,
                     (const float2*)(b->brp(x.q) + size_t(x.Hbb + n0 - L0H) * x.CP),
                     (const fmd::HbOsc*)(b->osc_tab[x.osc_slot].p + fmd_batch::kOscH + n0 - L0H), b->mix[x.q ^ 1].p, L0H,
                     x.CP);
}

/* The RDS decimator with one launch per stage; a chain in its normal regime collects its rolls. */
void stage_decimator_stages(Submit& x, hipStream_t sR)
{
  fmd_batch* const b = x.b;
  const fmd::Design& d = x.d;
  const unsigned C = x.C, CP = x.CP, q = unsigned(x.q);
  const unsigned* const hb_in = x.pl.hb_in;
  const fmd::HbMode* const hb_mode = x.pl.hb_mode;
  const dim3 rt(256);
  const float2* in = b->mix[q].p;
  for (size_t s = 0; s < d.hb.size(); s++)
  {
    const unsigned n_out =
        (d.hb[s].cic || d.hb[s].len == 11 || hb_mode[s] == fmd::HB_PASS) ? hb_in[s] / 2 : (hb_in[s] + 1) / 2;
    const bool last = (s + 1 == d.hb.size());
    float2* outp = last ? b->rdsraw[q].p : b->hbbuf[s].p;
    const unsigned Hout = last ? (x.T_lpf - 1) : unsigned(d.hb[s + 1].len - 1);
    const unsigned Hs = unsigned(d.hb[s].len - 1);
    float2* const hist_dst = s == 0 ? b->mix[q ^ 1].p : b->hbbuf[s - 1].p; // where the delay line lives
    if (hb_mode[s] == fmd::HB_PASS)
    { // unfiltered; the delay line stays (stage 0 keeps it in the other parity's buffer: copy it over)
      hipLaunchKernelGGL(fmd::k_hb_pass, x.rgrid(n_out), rt, 0, sR, in, Hs, outp, Hout, n_out, CP);
      if (s == 0)
        hipLaunchKernelGGL(fmd::k_roll<float2>, x.rgrid(Hs), rt, 0, sR, b->mix[q].p, b->mix[q ^ 1].p, Hs, 0u, CP);
      in = outp;
      continue;
    }
    if (d.hb[s].cic)
      hipLaunchKernelGGL(fmd::k_cic3, dim3(CP / 64, (n_out + 3) / 4), dim3(64, 4), 0, sR, in, outp, n_out, C, CP, Hout);
    else if (d.hb[s].len == 11)
      hipLaunchKernelGGL(fmd::k_halfband11, dim3(CP / 64, (n_out + 3) / 4), dim3(64, 4), 0, sR, in, outp, n_out,
                         b->hbcoef[s], C, CP, Hout);
    else if (b->dbg_hb4 && (d.hb[s].len - 1) / 2 >= 4 && d.hb[s].len <= 55)
      hipLaunchKernelGGL(fmd::k_halfband4, dim3(CP / 64, (n_out + 15) / 16), dim3(64, 4), 0, sR, in, outp, n_out,
                         d.hb[s].len, b->hbcoef[s], C, CP, Hout);
    else
      hipLaunchKernelGGL(fmd::k_halfband, dim3(CP / 64, (n_out + 4 * fmd::HB_R - 1) / (4 * fmd::HB_R)), dim3(64, 4), 0,
                         sR, in, outp, n_out, d.hb[s].len, b->hbcoef[s], C, CP, Hout);
    // keep the last L-1 input rows of this stage for the next call, then its input is free (stage 0: the tail of
    // mix[q] -> history rows of mix[q^1], which the next call's half-band reads)
    float2* const hist_src = s == 0 ? b->mix[q].p : b->hbbuf[s - 1].p;
    if (hb_mode[s] == fmd::HB_MIXED)
      hipLaunchKernelGGL(fmd::k_roll_hb_mixed, dim3((CP + 255) / 256), rt, 0, sR, in, (const float2*)outp, hist_dst, Hs,
                         hb_in[s], n_out, Hout, CP);
    else if (x.hb_all_normal)
      x.rolls.later(hist_src, hist_dst, Hs, hb_in[s]);
    else
      hipLaunchKernelGGL(fmd::k_roll<float2>, x.rgrid(Hs), rt, 0, sR, hist_src, hist_dst, Hs, hb_in[s], CP);
    in = outp;
  }
}

void stage_decimator(Submit& x, hipStream_t s)
{
  if (x.hbf_pl)
    stage_decimator_chain(x, s);
  else
    stage_decimator_stages(x, s);
}

/* The RDS 75-tap low-pass on stream s as a stage of the heavy part (layouts 0, 1 and the in-order schedule; layout 2:
 * launch_light_rds), with its input's roll: collected and flushed where the chain collects. */
void stage_rds_lpf(Submit& x, hipStream_t s)
{
  fmd_batch* const b = x.b;
  launch_ring(b, s, b->rdsraw[x.q].p, b->rlpf[x.q].p, x.R, x.T_lpf, b->rds_lpf_taps.p, b->rds_lpf_g, b->dbg_ring4 != 0,
              0u, x.rds_org);
  if (x.hb_all_normal)
  {
    x.rolls.later(b->rdsraw[x.q].p, b->rdsraw[x.q ^ 1].p, x.T_lpf - 1, x.R);
    x.rolls.flush(x.CP, s);
  }
  else
    hipLaunchKernelGGL(fmd::k_roll<float2>, x.rgrid(x.T_lpf - 1), dim3(256), 0, s, b->rdsraw[x.q].p,
                       b->rdsraw[x.q ^ 1].p, x.T_lpf - 1, x.R, x.CP);
}

/* The ring resampler's plan kernel (tap tables of this call's phases: no input but the positions), once per call. */
void stage_rs_plan(Submit& x, hipStream_t s)
{
  fmd_batch* const b = x.b;
  if (!x.ring || x.rs_planned)
    return;
  x.rs_planned = true;
  auto plan = b->rsr_R == 4 ? &fmd::k_rs_plan<4, 4> : b->rsr_NW == 8 ? &fmd::k_rs_plan<2, 8> : &fmd::k_rs_plan<2, 4>;
  hipLaunchKernelGGL(plan, dim3(x.rs_steps * b->rsr_NW), dim3(64), 0, s, b->rs_coeff.p, x.d.rs_order, b->rs_pos,
                     x.d.rs_step, x.A, b->rsr_rb, b->rsr_nbr, b->rsr_tab.p, b->rsr_nbm, b->rsr_head.p, b->rsr_steps.p);
}

/* The resampler in its ring form (k_resample_ring, behind its plan kernel) */
void stage_resampler_ring(Submit& x, hipStream_t s)
{
  fmd_batch* const b = x.b;
  // one workgroup (a whole CU's LDS) for every CU the serial stage leaves free: one round, with an equal
  // run of (group, step) units each, >= 8 steps (measured with 160 / 176 / 184 / 192 of 192: 267 800 /
  // 278 700 / 280 000 / 282 300 MS/s whole path on one box)
  const unsigned groups = x.CP / 64;
  const unsigned ncu = unsigned(b->n_cus) - ((b->serial_exclusive && !x.serial_mode) ? (groups + 1) / 2 : 0u);
  const unsigned units = groups * x.rs_steps;
  unsigned W = std::max(1u, ncu);
  W = std::max(1u, std::min(W, units / 8u));
  const unsigned per_wg = (units + W - 1) / W;
  W = (units + per_wg - 1) / per_wg;
  const unsigned lds = b->rsr_nbr * 4096u;
  // wave priority in the overlapped pipeline (the half-band chain's stays 0)
  const unsigned prio = (!x.serial_mode && b->concurrency == 2) ? 2u : 0u;
  stage_rs_plan(x, s); // (already done in front of the half-band chain where the schedule put it there)
  auto go = [&](auto kern) {
    launch(kern, dim3(W), dim3(64, b->rsr_NW + 1), lds, s, x.timed(8), x.timed(9), b->brp(x.q), x.Hbb, b->rsr_rb,
           x.d.rs_order, b->rsr_tab.p, b->rsr_nbm, b->rsr_head.p, b->rsr_steps.p, x.rs_steps, per_wg, b->rsr_nbr, x.A,
           b->rs[x.q].p, x.T_alp - 1, x.C, x.CP, prio);
  };
  if (b->rsr_R == 4)
    go(&fmd::k_resample_ring<4, 4>);
  else if (b->rsr_NW == 8 && b->params.fir_reduction == 2)
    go(&fmd::k_resample_ring<2, 8, true>); // FMD_FIR_FMA_PARITY_WAIVED
  else if (b->rsr_NW == 8)
    go(&fmd::k_resample_ring<2, 8>);
  else
    go(&fmd::k_resample_ring<2, 4>);
}

/* ... and in its window-per-wave form (k_rs_table + k_resample) */
void stage_resampler_window(Submit& x, hipStream_t s)
{
  fmd_batch* const b = x.b;
  hipLaunchKernelGGL(fmd::k_rs_table, dim3(x.A), dim3(64), 0, s, b->rs_coeff.p, x.d.rs_order, b->rs_pos, x.d.rs_step,
                     x.A, b->ktab.p, b->rs_row, b->rs_margin, b->pidx.p);
  hipLaunchKernelGGL(fmd::k_resample, dim3(x.CP / 64, (x.A + 4 * fmd::RS_R - 1) / (4 * fmd::RS_R)), dim3(64, 4), 0, s,
                     b->brp(x.q), x.Hbb, x.d.rs_order, b->ktab.p, b->rs_row, b->rs_margin, b->pidx.p, x.A, b->rs[x.q].p,
                     x.T_alp - 1, x.C, x.CP);
}

/* The multiplex rows of the call (the _mpx entry points): br[q]'s data rows, transposed, next to the resampler
 * that reads the same rows.  In front of EV_HEAVY on every path: the next writer of these rows, the serial stage
 * of the next-but-one call, runs behind that call's IF FIR, which waits for this EV_HEAVY; EV_ROLL behind it is
 * what fmd_batch_wait and the caller's stream wait for. */
void stage_mpx(Submit& x, hipStream_t s)
{
  fmd_batch* const b = x.b;
  const Out& mpx = x.c.mpx;
  if (!mpx.p)
    return;
  const unsigned M = x.M, CP = x.CP, tiles = (M + fmd::MPX_T - 1) / fmd::MPX_T;
  const float* rows = reinterpret_cast<const float*>(b->brp(x.q) + size_t(x.Hbb) * CP);
  // (fmd_batch_debug_mpx_ms: the kernel's own start and stop, events of the call's slot)
  const hipEvent_t t0 = b->dbg_mpx_timing ? b->mpx_ev[x.es][0].e : nullptr;
  const hipEvent_t t1 = b->dbg_mpx_timing ? b->mpx_ev[x.es][1].e : nullptr;
  write_rows(
      b, b->sel[FMT_MPX], s,
      [&](const int2* ent, unsigned n) { // (fmd_batch_select_mpx): tiles of 64 entries
        const dim3 g((n + 63) / 64, tiles);
        b->mpx_ev[x.es][0].in_use = t0 != nullptr;
        if (mpx.fmt == FMD_MPX_S16)
          launch(fmd::k_mpx_out_sel<fmd::MpxS16>, g, dim3(256), 0, s, t0, t1, rows, M, n, CP, ent,
                 static_cast<int16_t*>(mpx.p), mpx.stride);
        else
          launch(fmd::k_mpx_out_sel<fmd::MpxF32>, g, dim3(256), 0, s, t0, t1, rows, M, n, CP, ent,
                 static_cast<float*>(mpx.p), mpx.stride);
      },
      [&] {
        const dim3 g(CP / 64, tiles);
        b->mpx_ev[x.es][0].in_use = t0 != nullptr;
        if (mpx.fmt == FMD_MPX_S16)
          launch(fmd::k_mpx_out<fmd::MpxS16>, g, dim3(256), 0, s, t0, t1, rows, M, x.C, CP,
                 static_cast<int16_t*>(mpx.p), mpx.stride);
        else
          launch(fmd::k_mpx_out<fmd::MpxF32>, g, dim3(256), 0, s, t0, t1, rows, M, x.C, CP, static_cast<float*>(mpx.p),
                 mpx.stride);
      });
}

/* The resampler in the call's form and the multiplex writer beside it; the baseband rows' roll is collected. */
void stage_resampler(Submit& x, hipStream_t s)
{
  if (x.ring)
    stage_resampler_ring(x, s);
  else
    stage_resampler_window(x, s);
  stage_mpx(x, s);
  x.rolls.later(x.b->brp(x.q), x.b->brp(x.q ^ 1), x.Hbb, x.M);
}

/* The audio 29-tap low-pass on stream s as a stage of the heavy part (layout 2: launch_light_audio); its input's roll
 * goes out with everything collected so far. */
void stage_audio_lpf(Submit& x, hipStream_t s)
{
  fmd_batch* const b = x.b;
  launch_ring(b, s, b->rs[x.q].p, b->alp[x.q].p, x.A, x.T_alp, b->audio_taps.p, b->alpf_g, b->dbg_ring4 != 0, 0u,
              nullptr);
  x.rolls.later(b->rs[x.q].p, b->rs[x.q ^ 1].p, x.T_alp - 1, x.A);
  x.rolls.flush(x.CP, s);
}

/* The front of every call, in both schedules: the uploads, the IF stage with the channel IQ behind it, the serial
 * stage. */
int submit_front(Submit& x)
{
  const Event *ce = x.ce, *pe2 = x.pe2;
  upload_oscillator(x);
  upload_walk(x);
  /* The input is ready in the order of the caller's stream.  Where that stream has nothing pending (the usual case:
   * the host has just synchronised it for the previous outputs, or never uses it for anything else) the input IS
   * ready and no event has to carry that: one record in the caller's queue and one barrier packet in front of the IF
   * FIR less per call (+1.5 % whole path on the null stream, round 6). */
  const bool input_pending = x.serial_mode ? false : hipStreamQuery(x.stream) != hipSuccess;
  (void)hipGetLastError(); // (hipErrorNotReady is an answer, not an error)
  if (input_pending)
  {
    x.signal(ce[fmd_batch::EV_IN], x.stream);
    x.after(x.sF, ce[fmd_batch::EV_IN]);
  }
  if (x.have_prev2)
  {
    // (demod[q] was last read by the serial stage two calls ago: EV_SER of that call -- implied by its EV_HEAVY below,
    // the heavy part starts behind the serial stage; not where an energy experiment leaves the heavy part out)
    if (x.stage_mask != 63u)
      x.after(x.sF, pe2[fmd_batch::EV_SER]);
    // Also run behind the bandwidth-heavy part of the post chain of two calls ago (half-band chain, resampler):
    // side by side with those the FIR and they were both ~25 % slower.  The rest of that chain (the light part) is
    // lane-per-channel work that leaves most CUs idle: the FIR runs beside it.  (Behind the RDS half only, or
    // through a word in device memory instead of the event: measured in rounds 3 and 5, the period did not move --
    // docs/MEASUREMENTS.md.)
    x.after(x.sF, pe2[fmd_batch::EV_HEAVY]);
  }
  // a batch that is one of several sub-batches sharing these streams (fmd_batch_create above 8192 channels): the
  // FIR also stays behind the heavy part of the sub-batch call two back in the common sequence
  if (x.b->sched_prev2)
    x.after(x.sF, x.b->sched_prev2);
  if (int rc = stage_if(x)) // cannot happen: the geometry was checked when the batch was created
  {
    mark_failed(x.b, "the IF stage refused a call after events were recorded");
    return rc;
  }
  // the level meter behind the FIR also reads the input, and EV_INDONE covers the channel IQ's rows: it is what
  // tells the caller its buffer is free, and what fmd_batch_wait and the caller's stream wait for
  launch_ciq(x.b, x.c.ciq, x.q, x.M, x.sF);
  x.signal(ce[fmd_batch::EV_INDONE], x.sF);

  // br[q] / mix[q] were last read by the resampler / first half-band two calls ago: this call's FIR already waited
  // for that call's heavy part (EV_HEAVY above), so EV_FIR covers them.  EV_HEAVY is recorded in FRONT of the history
  // rolls behind the heavy part (the FIR starts earlier); the rolls read the tails of br[q] / mix[q]: EV_ROLL
  if (x.have_prev2)
    x.after(x.sS, pe2[fmd_batch::EV_ROLL]);
  x.after(x.sS, ce[fmd_batch::EV_FIR]);
  stage_serial(x);
  x.signal(ce[fmd_batch::EV_SER], x.sS);
  x.mark(2);
  return FMD_OK;
}

/* The post chain: "heavy" = bandwidth / LDS bound and filling the chip (decimator, resampler, in some layouts the two
 * complex low-pass filters), "light" = lane-per-channel recurrences on CP / 64 workgroups (launch_light_rds,
 * launch_light_audio).
 *
 * In order: the stage order of the reference, which the per-stage profile is keyed to -- everything on the caller's
 * stream (concurrency 0, profiling level 2), or "split_post": the RDS chain on s_rds beside the audio chain on s_post
 * (a batch of one or two wavefronts). */
void submit_in_order(Submit& x)
{
  const Event* ce = x.ce;
  const hipStream_t sR = x.sR, sA = x.sA;
  const bool two = sA != sR && !x.serial_mode;

  x.after(sR, ce[fmd_batch::EV_SER]);
  // Without mixed rows stage 0 reads the last L0H history rows of br[q]: the PREVIOUS call's roll wrote
  // them, on the audio stream.  One stream: stream order.  Two: its EV_ROLL.
  if (x.nomix && two && x.ci > 1)
    x.after(sR, x.pe1[fmd_batch::EV_ROLL]);
  stage_post_delay(x, sR);
  stage_decimator(x, sR);
  x.mark(3);
  if (x.hbf_pl && x.nomix)
    stage_mix_tail(x, sR);
  stage_rds_lpf(x, sR);
  x.mark(4);
  if (two && x.ci > 1) // call k-1's status record copies the RDS state this call's bit recovery writes
    x.prev_aud = x.pe1[fmd_batch::EV_AUD];
  launch_light_rds(x, sR); // (records EV_RDS)
  x.mark(5);

  if (two) // (one stream: the RDS branch in front has waited)
    x.after(sA, ce[fmd_batch::EV_SER]);
  stage_resampler(x, sA);
  x.mark(6);
  stage_audio_lpf(x, sA);
  x.mark(7);
  x.audio_after = -1; // behind its resampler and low-pass in stream order
  x.status_after_rds = sA != sR;
  launch_light_audio(x, sA); // (records EV_AUD)
  x.mark(8);
  x.signal(ce[fmd_batch::EV_HEAVY], sA);
  x.signal(ce[fmd_batch::EV_ROLL], sA);
}

/* Overlapped: both heavy parts first on the post stream, the light parts behind them on streams of their own: the
 * next call's FIR runs beside the light parts, and the next call's heavy parts do not queue behind them (rlpf / alp,
 * the buffers between a heavy and a light part, are double-buffered by call parity; their readers of two calls ago
 * are long done).
 *
 * Where the post chain's two complex low-pass filters (RDS 75 taps, audio 29 taps: ~0.05 ms each alone at 8192
 * channels, a few hundred small workgroups) and the light part run -- the stream layout ("lpf_late" of
 * fmd_batch_debug_set overrides the choice):
 *   0  both filters on the heavy stream (the RDS one between half-band chain and resampler, the audio one behind
 *      the resampler), the light part on one stream behind them.  Long IF filters (> 512 taps): there the IF
 *      FIR alone sets the period and more streams only get in its way (config 5, round 6, one box: 86 500 MS/s
 *      against 80 800 with layout 2; the streams' heads wait for events in hardware queues the FIR's shares).
 *   1  the filters on a stream of their own (s_lpf), each behind the kernel that feeds it (EV_DEC: the
 *      decimator; EV_HEAVY: the resampler), the light part on one stream: round 4's layout -- the IF FIR at
 *      0.62-0.65 of the HBM peak inside the pipeline, the whole path 4 % slower than layout 2.
 *   2  no filter on the heavy stream or beside the next IF FIR's start: the RDS low-pass at the head of the light
 *      part's RDS half (s_rds, behind EV_DEC), the audio low-pass at the head of its audio half on s_lpf (behind
 *      EV_HEAVY) -- two chains of lane-per-channel kernels side by side, each shorter than a period.  Default
 *      for short IF filters: +2.3 % at the driver's flags over layout 1.
 * The filters' inputs (rdsraw, rs) are buffered by call parity, so the next call's decimator / resampler need
 * not wait for them. */
void submit_overlapped(Submit& x)
{
  fmd_batch* const b = x.b;
  const Event *ce = x.ce, *pe2 = x.pe2;
  const hipStream_t sP = x.sP, sL = x.sL, sl = b->s_lpf;
  const int layout = x.layout;
  const bool decimate = (x.stage_mask & 4u) != 0, resample = (x.stage_mask & 8u) != 0; // (the energy experiment)
  const bool mix_tail = decimate && x.hbf_pl && x.nomix;

  if (x.have_prev2)
  {
    x.after(sP, pe2[fmd_batch::EV_RDS]);
    x.after(sP, pe2[fmd_batch::EV_AUD]);
    if (layout != 0) // rdsraw[q] is written again: its low-pass of two calls ago has read it
      x.after(sP, pe2[fmd_batch::EV_RDSH]);
    if (layout == 1) // ... and rs[q] (layout 2: its reader is in front of EV_AUD, waited for above)
      x.after(sP, pe2[fmd_batch::EV_ALP]);
  }
  if (layout != 0)
    stage_rs_plan(x, sP); // off the path between the half-band chain and the resampler
  if (decimate)
  {
    x.after(sP, ce[fmd_batch::EV_SER]);
    stage_post_delay(x, sP);
    stage_decimator(x, sP);
    if (layout != 0)
    { // the low-pass is not the heavy stream's; the decimator's rolls wait for the resampler's: one launch behind
      // EV_HEAVY (k_roll_set takes four)
      if (x.rolls.n > 3)
        x.rolls.flush(x.CP, sP);
    }
    else
    {
      if (mix_tail)
        stage_mix_tail(x, sP);
      stage_rds_lpf(x, sP);
    }
  }
  x.signal(ce[layout != 0 ? fmd_batch::EV_DEC : fmd_batch::EV_RDSH], sP);
  if (resample)
  {
    stage_resampler(x, sP);
    if (layout == 0)
      stage_audio_lpf(x, sP);
  }
  x.signal(ce[fmd_batch::EV_HEAVY], sP); // the next-but-one call's IF FIR may go
  if (mix_tail && layout != 0)
    stage_mix_tail(x, sP);
  x.rolls.flush(x.CP, sP); // (layouts 1, 2: the history rolls of both heavy parts in one launch)
  x.signal(ce[fmd_batch::EV_ROLL], sP);
  if (layout == 1)
  { // the two low-pass filters on their own stream
    if (x.have_prev2)
    { // rlpf[q] / alp[q] were last read by the light part of two calls ago
      x.after(sl, pe2[fmd_batch::EV_RDS]);
      x.after(sl, pe2[fmd_batch::EV_AUD]);
    }
    x.after(sl, ce[fmd_batch::EV_DEC]);
    if (decimate)
      stage_rds_lpf(x, sl);
    x.signal(ce[fmd_batch::EV_RDSH], sl);
    x.after(sl, ce[fmd_batch::EV_HEAVY]);
    if (resample)
      stage_audio_lpf(x, sl);
    x.signal(ce[fmd_batch::EV_ALP], sl);
  }
  /* The light part goes out at once: its RDS half behind the RDS half of the heavy part (it runs beside the
   * resampler), the audio tail behind the whole heavy part.  (Until round 3 it was kept back until the NEXT
   * call's serial stage had ended, so that it ran beside that call's heavy part and not beside a FIR -- built
   * again and measured in round 5: the FIR gains 0.02 of the HBM peak, the whole path loses 7.5 %; removed.) */
  // layout 2: the audio half on the stream the filters have in layout 1, beside the RDS half
  const hipStream_t s_aud = layout == 2 ? sl : sL;
  x.tl0 = x.timed(4);
  x.tl1 = x.timed(5);
  if (layout != 2)
    x.after(sL, ce[fmd_batch::EV_RDSH]);
  if (x.stage_mask & 16u)
  {
    if (s_aud != sL && x.ci > 1) // call k-1's status record copies the RDS state this call's bit recovery writes
      x.prev_aud = x.pe1[fmd_batch::EV_AUD];
    launch_light_rds(x, sL); // (layout 2: behind EV_DEC; records EV_RDS)
  }
  else
    x.signal(ce[fmd_batch::EV_RDS], sL);
  x.audio_after = layout == 1 ? fmd_batch::EV_ALP : fmd_batch::EV_HEAVY;
  x.status_after_rds = s_aud != sL;
  if (x.stage_mask & 32u)
    launch_light_audio(x, s_aud); // (records EV_AUD)
  else
    x.signal(ce[fmd_batch::EV_AUD], s_aud);
}

/* The call is submitted: its index goes into the batch together with the positions the host tracks. */
void commit_call(Submit& x)
{
  fmd_batch* const b = x.b;
  const Call& c = x.c;
  const fmd::CallPlan& pl = x.pl;
  b->call_index = x.ci;
  b->slot_call[x.es] = x.ci;
  if (x.evset)
    b->prof_calls++;
  if (!c.ciq_in())
  { // (channel IQ rows as input: the IF stage did not run -- its decimator phase, tuner phase and history stay)
    b->if_pos = pl.if_pos;                                    // DownConvert.cpp:132
    b->lut_idx = (b->lut_idx + c.samples) % x.d.table_size;   // FmDecode.cpp:81
    b->hist_sel ^= 1;
  }
  b->rs_pos = pl.rs_pos;                                      // DownConvert.cpp:230-232
  b->osc_re = x.osc_re;                                       // DownConvert.cpp:440-441 (batch-wide, see osc_on)
  b->osc_im = x.osc_im;
  b->osc_warm -= std::min(b->osc_warm, x.M);
  b->rds_lpf_g = (b->rds_lpf_g + x.R) % x.T_lpf;
  b->mf_g = (b->mf_g + x.R) % x.T_mf;
  b->alpf_g = (b->alpf_g + x.A) % x.T_alp;
  b->lastM = x.M;
  b->lastA = x.A;
  b->lastR = x.R;
  if (c.audio.out)
    *c.audio.out = 2 * x.A;
  if (c.mpx.out)
    *c.mpx.out = c.mpx.p ? x.M : 0;
  if (c.feed.p)
    b->feed_g += x.A;
  if (b->loud_bf)
  { // the meter's frame count (mode-1 calls only: a mode-0 call is a splice) and what a lagged collect may take
    if (b->loud_mode)
      b->loud_g += x.A;
    for (int k = 4; k > 0; k--)
      b->loud_done[k] = b->loud_done[k - 1];
    b->loud_done[0] = b->loud_g / b->loud_bf;
  }
  if (c.feed.out)
    *c.feed.out = (c.feed.p && c.feed.deliver) ? pl.feed_n : 0;
  if (c.ciq.out)
    *c.ciq.out = c.ciq.p ? x.M : 0;
}

/* One call of a batch with buffers of its own: checked, then submitted stage by stage in the schedule of its stream
 * layout, then committed.  tests/test_call_trace_cpu.py is the record of what that puts on which stream. */
int submit_call(fmd_batch* b, const Call& c)
{
  fmd::CallPlan pl;
  if (int rc = check_call(b, c, pl))
    return rc;
  Submit x(b, c, pl);
  if (int rc = take_profiling_events(x))
    return rc;
  decide_forms(x);
  if (int rc = submit_front(x))
    return rc;
  if (x.serial_mode || b->split_post)
    submit_in_order(x);
  else
    submit_overlapped(x);
  x.mark(9);
  if (!x.serial_mode && b->concurrency < 2)
  { // order the caller's stream after everything this call launched
    x.note(hipStreamWaitEvent(x.stream, x.ce[fmd_batch::EV_AUD], 0));
    x.note(hipStreamWaitEvent(x.stream, x.ce[fmd_batch::EV_RDS], 0));
    x.note(hipStreamWaitEvent(x.stream, x.ce[fmd_batch::EV_INDONE], 0));
    x.note(hipStreamWaitEvent(x.stream, x.ce[fmd_batch::EV_ROLL], 0));
  }
  x.note(hipGetLastError());
  if (x.herr != hipSuccess)
  { // part of the call is on the device, part is not: histories and channel state no longer line up
    b->failed = true;
    b->fail_msg = std::string("a call broke off while it was being submitted: ") + hipGetErrorString(x.herr);
    return fail(FMD_ERR_DEVICE, b->fail_msg);
  }
  commit_call(x);
  return FMD_OK;
}

} // namespace
