/*
 * call_trace.cpp -- the driver of tests/test_call_trace_cpu.py: submits process calls through the C ABI of
 * include/fmd.h in every concurrency mode, stream layout, kernel form and entry point, linked against the recording
 * double of the HIP runtime (hip_recorder.cpp).  It prints, per scenario, a "== name" line and every runtime call the
 * library made (setup calls included), with a "-- call" line in front of every process call; the test reduces that
 * to the last call's trace and a hash of the whole.  No kernel runs and no GPU is opened.
 */
#include "fmd.h"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" void rec_on(int);
extern "C" void rec_busy(int);
extern "C" void rec_epoch();
extern "C" void* rec_stream();
extern "C" void rec_kernels();

namespace
{
[[noreturn]] void die(const char* what, int rc)
{
  printf("FAILED %s: rc %d: %s\n", what, rc, fmd_last_error());
  exit(1);
}
#define OK(x)                                                                                                          \
  do                                                                                                                   \
  {                                                                                                                    \
    const int rc_ = (x);                                                                                               \
    if (rc_ < 0)                                                                                                       \
      die(#x, rc_);                                                                                                    \
  } while (0)

fmd_params geometry(double fs, unsigned D, unsigned order = 0, unsigned table = 0)
{
  fmd_params p{};
  p.sample_rate_if = fs;
  p.tuning_offset = -0.15 * fs;
  p.sample_rate_pcm = 48000.0;
  p.bandwidth_pcm = 15000.0;
  p.downsample = D;
  p.table_size = table;
  p.if_filter_order = order;
  return p;
}
const fmd_params kRef = geometry(2.4e6, 11, 88, 64); // the reference geometry

/* "device" rows for every output of a call; sized for the largest call (the double's memory is the host's, untouched
 * pages cost nothing) */
void* rows(size_t bytes)
{
  void* p = nullptr;
  if (posix_memalign(&p, 64, bytes ? bytes : 64))
    die("posix_memalign", -1);
  return p;
}
size_t up16(size_t n) { return (n + 15) / 16 * 16; }
const char* nm(const char* f, ...) // a scenario's name
{
  static char buf[128];
  va_list a;
  va_start(a, f);
  vsnprintf(buf, sizeof buf, f, a);
  va_end(a);
  return buf;
}

/* ragged call sizes: never four equal calls */
const unsigned kSizes[4] = {65536, 48000, 65530, 33334};

struct Run
{
  fmd_batch* b = nullptr;
  unsigned C = 0, maxN = 65536;
  void *iq = nullptr, *audio = nullptr, *mpx = nullptr, *feed = nullptr, *ciq = nullptr;
  size_t sa = 0, sm = 0, sf = 0;
  void* stream = nullptr;
  // what the next calls ask for
  int iq_fmt = FMD_IQ_F32, pcm = FMD_PCM_F32;
  int want_mpx = -1, want_feed = -1, want_ciq = -1; // -1 off, else the format
  size_t iq_stride = 0;                             // 0: one shared capture

  Run(const char* name, const fmd_params& p, unsigned channels, int conc, unsigned max_samples = 65536)
      : C(channels), maxN(max_samples)
  {
    printf("== %s\n", name);
    rec_epoch();
    rec_on(1);
    OK(fmd_batch_create(&p, C, nullptr, 0, nullptr, nullptr, &b));
    if (conc >= 0)
      OK(fmd_batch_set_concurrency(b, conc));
    sa = up16(fmd_batch_max_audio_floats(b, maxN));
    sm = up16(fmd_batch_max_mpx_samples(b, maxN));
    iq = rows(size_t(4) * maxN * 8); // up to four captures of float IQ
    audio = rows(sa * C * 4);
    mpx = rows(sm * C * 4);
    ciq = rows(sm * C * 8);
  }
  Run(const Run&) = delete;
  ~Run()
  {
    fmd_batch_destroy(b);
    rec_on(0);
    free(iq);
    free(audio);
    free(mpx);
    free(feed);
    free(ciq);
  }
  void scenario(const char* name) { printf("== %s\n", name); }
  void key(const char* k, int v) { OK(fmd_batch_debug_set(b, k, v)); }
  void feed_on(int divisor)
  {
    OK(fmd_batch_set_feed(b, divisor));
    sf = up16(fmd_batch_max_feed_samples(b, maxN));
    free(feed);
    feed = rows(sf * C * 4);
  }
  fmd_call record(unsigned n) const
  {
    fmd_call c{};
    c.size = sizeof(c);
    c.iq = iq;
    c.iq_format = iq_fmt;
    c.iq_channel_stride = iq_stride;
    c.samples = n;
    c.audio = {audio, pcm, sa, nullptr};
    if (want_mpx >= 0)
      c.mpx = {mpx, want_mpx, sm, nullptr};
    if (want_feed >= 0)
      c.feed = {feed, want_feed, sf, nullptr};
    if (want_ciq >= 0)
      c.ciq = {ciq, want_ciq, sm, nullptr};
    c.stream = stream;
    return c;
  }
  void call(unsigned n)
  {
    printf("-- call %u samples\n", n);
    const fmd_call c = record(n);
    OK(fmd_batch_process_device_call(b, &c));
  }
  void calls(const unsigned* sizes = kSizes, int n = 4)
  {
    for (int i = 0; i < n; i++)
      call(sizes[i]);
  }
  void wait(bool pending = false) // pending: the events have not completed, fmd_batch_wait orders the stream behind them
  {
    rec_busy(pending);
    OK(fmd_batch_wait(b, stream));
    rec_busy(0);
  }
};

void basic_modes()
{
  const unsigned Cs[2] = {64, 192}; // split_post by default, and not
  for (unsigned C : Cs)
    for (int conc = 0; conc < 3; conc++)
      for (int prof = 0; prof < 3; prof++)
      {
        Run r(nm("basic C=%u concurrency=%d profiling=%d", C, conc, prof), kRef, C, conc);
        OK(fmd_batch_set_profiling(r.b, prof));
        r.calls();
        r.wait(prof == 0 && C == 192);
      }
}

void layouts()
{
  for (int l = 0; l < 3; l++)
  {
    Run r(nm("layout C=192 lpf_late=%d", l), kRef, 192, 2);
    r.key("lpf_late", l);
    r.calls();
    r.wait();
  }
  {
    Run r("layout C=192 lpf_late alternating per call", kRef, 192, 2);
    for (int i = 0; i < 6; i++)
    {
      r.key("lpf_late", i % 3);
      r.call(kSizes[i % 4]);
    }
    r.wait();
  }
  {
    Run r("layout C=192 stage_mask 1", kRef, 192, 2);
    r.key("stage_mask", 1);
    r.calls();
    r.scenario("layout C=192 stage_mask 63 behind 1");
    r.key("stage_mask", 63);
    r.calls();
    r.wait();
  }
  for (int m = 2; m <= 32; m *= 2)
  {
    Run r(nm("layout C=192 stage_mask %d", m), kRef, 192, 2);
    r.key("stage_mask", m);
    r.calls(kSizes, 3);
  }
  {
    Run r("layout C=192 split_post=1 halfband_chain=1", kRef, 192, 2);
    r.key("split_post", 1);
    r.key("halfband_chain", 1);
    r.calls();
    r.wait();
  }
}

void chain_and_ring_small()
{
  for (int conc = 1; conc <= 2; conc++)
    for (int nomix = 0; nomix < 2; nomix++)
    {
      Run r(nm("small C=64 concurrency=%d halfband_chain=1 nomix=%d", conc, nomix), kRef, 64, conc);
      r.key("halfband_chain", 1);
      r.key("nomix", nomix);
      r.calls();
      r.wait();
    }
  for (int form = 0; form < 3; form++)
  {
    Run r(nm("small C=64 resampler=1 rsr_form=%d", form), kRef, 64, 2);
    r.key("rsr_form", form);
    r.key("resampler", 1);
    r.calls();
    r.wait();
  }
  {
    Run r("small C=192 halfband_chain=1 resampler=1 lpf_late=1", kRef, 192, 2);
    r.key("halfband_chain", 1);
    r.key("resampler", 1);
    r.key("lpf_late", 1);
    r.calls();
    r.scenario("small C=192 halfband_chain=1 resampler=1 lpf_late=0");
    r.key("lpf_late", 0);
    r.calls();
    r.scenario("small C=192 halfband_chain=1 resampler=1 lpf_late=2 nomix=0");
    r.key("lpf_late", 2);
    r.key("nomix", 0);
    r.calls();
    r.wait();
  }
  {
    fmd_params p = kRef;
    p.fir_reduction = FMD_FIR_FMA_PARITY_WAIVED;
    Run r("small C=64 fir_reduction FMA, resampler=1", p, 64, 2);
    r.key("resampler", 1);
    r.calls();
    r.wait();
  }
  {
    Run r("small C=64 hb4=0 ring4=0 halfband_chain=0", kRef, 64, 2);
    r.key("hb4", 0);
    r.key("ring4", 0);
    r.key("halfband_chain", 0);
    r.calls();
    r.wait();
  }
}

void large_batch()
{
  {
    Run r("large C=8192 concurrency=1", kRef, 8192, 1);
    r.calls();
    r.wait();
  }
  Run r("large C=8192 concurrency=2", kRef, 8192, 2);
  r.calls();
  const struct
  {
    const char* key;
    int v;
  } forms[] = {{"serial_claim", 1}, {"fir_nt", 1}, {"fir_nt", 3}, {"fir_ro", 1}, {"fir_ro", 3}, {"fir_ro", -2},
               {"nomix", 0}, {"serial_exclusive", 0}};
  for (const auto& f : forms)
  {
    r.scenario(nm("large C=8192 then %s=%d", f.key, f.v));
    r.key(f.key, f.v);
    r.calls();
  }
  r.wait();
}

void sub_batches()
{
  for (int conc = 1; conc <= 2; conc++)
  {
    Run r(nm("sub-batches C=8200 concurrency=%d", conc), kRef, 8200, conc);
    r.want_mpx = FMD_MPX_F32;
    rec_busy(conc == 1); // (mode 1: the shell orders the caller's stream behind the events that are still pending)
    r.calls();
    rec_busy(0);
    r.wait(true);
  }
}

/* the positional entry points, which build the same record */
void positional(Run& r, unsigned n, int which, int fmt)
{
  printf("-- call %u samples\n", n);
  unsigned na = 0, nm = 0, nf = 0;
  if (which == 0)
    OK(fmd_batch_process_device_mpx(r.b, r.iq, r.iq_fmt, 0, n, r.audio, r.pcm, r.sa, &na, r.mpx, fmt, r.sm, &nm,
                                    r.stream));
  else
    OK(fmd_batch_process_device_feed(r.b, r.iq, r.iq_fmt, 0, n, r.audio, r.pcm, r.sa, &na, r.mpx, FMD_MPX_S16, r.sm,
                                     &nm, r.feed, fmt, r.sf, &nf, r.stream));
}

void inputs_and_outputs()
{
  const struct
  {
    const char* name;
    int fmt;
  } iqf[] = {{"u8", FMD_IQ_U8}, {"s8", FMD_IQ_S8}, {"s16", FMD_IQ_S16}};
  for (const auto& f : iqf)
    for (unsigned C : {192u, 8192u})
    {
      Run r(nm("io C=%u iq %s", C, f.name), kRef, C, 2);
      r.iq_fmt = f.fmt;
      r.calls();
      r.wait();
    }
  for (unsigned C : {64u, 192u})
  {
    Run r(nm("io C=%u pcm s16", C), kRef, C, 2);
    r.pcm = FMD_PCM_S16;
    r.calls();
    r.wait();
  }
  for (unsigned C : {64u, 192u})
    for (int fmt = 0; fmt < 2; fmt++)
    {
      Run r(nm("io C=%u _mpx format %d", C, fmt), kRef, C, 2);
      for (unsigned n : kSizes)
        positional(r, n, 0, fmt);
      r.wait();
    }
  for (unsigned C : {64u, 192u})
    for (int fmt = 0; fmt < 2; fmt++)
    {
      Run r(nm("io C=%u _feed format %d divisor %d", C, fmt, 2 + fmt), kRef, C, 2);
      r.feed_on(2 + fmt);
      for (unsigned n : kSizes)
        positional(r, n, 1, fmt);
      r.wait();
    }
  for (unsigned C : {64u, 192u})
    for (int fmt = 0; fmt < 2; fmt++)
    {
      Run r(nm("io C=%u _call ciq format %d", C, fmt), kRef, C, 2);
      r.want_ciq = fmt;
      r.calls();
      r.wait();
    }
  for (int pcm = 0; pcm < 2; pcm++)
  {
    Run r(nm("io C=192 select audio only, pcm format %d", pcm), kRef, 192, 2);
    r.pcm = pcm;
    const unsigned a[2] = {191, 3};
    OK(fmd_batch_select_audio(r.b, a, 2));
    r.calls();
    r.wait();
  }
  { // every output at once, then with every selection on, then with the selections changed while events are pending
    Run r("io C=192 all outputs", kRef, 192, 2);
    r.feed_on(3);
    r.pcm = FMD_PCM_S16;
    r.want_mpx = FMD_MPX_F32;
    r.want_feed = FMD_FEED_S16;
    r.want_ciq = FMD_CIQ_F32;
    r.calls();
    const unsigned a[3] = {5, 100, 191}, m[2] = {7, 0}, f[4] = {1, 2, 3, 190}, q[1] = {64};
    r.scenario("io C=192 select audio");
    OK(fmd_batch_select_audio(r.b, a, 3));
    r.calls();
    r.scenario("io C=192 select audio + mpx");
    OK(fmd_batch_select_mpx(r.b, m, 2));
    r.calls();
    r.scenario("io C=192 select audio + mpx + feed");
    OK(fmd_batch_select_feed(r.b, f, 4));
    r.calls();
    r.scenario("io C=192 select audio + mpx + feed + ciq");
    OK(fmd_batch_select_ciq(r.b, q, 1));
    r.calls();
    r.scenario("io C=192 selections changed in front of every call, events pending: the pools grow");
    r.pcm = FMD_PCM_F32;
    r.want_mpx = FMD_MPX_S16;
    r.want_feed = FMD_FEED_F32;
    r.want_ciq = FMD_CIQ_S16;
    rec_busy(1);
    for (int i = 0; i < 4; i++)
    {
      OK(fmd_batch_select_audio(r.b, a, 1 + i % 3));
      OK(fmd_batch_select_mpx(r.b, m, 1 + i % 2));
      OK(fmd_batch_select_feed(r.b, f, 1 + i));
      OK(fmd_batch_select_ciq(r.b, a, 1 + i % 3));
      r.call(kSizes[i]);
    }
    rec_busy(0);
    r.scenario("io C=192 selections off again");
    OK(fmd_batch_select_audio(r.b, nullptr, 0));
    OK(fmd_batch_select_mpx(r.b, nullptr, 0));
    OK(fmd_batch_select_feed(r.b, nullptr, 0));
    OK(fmd_batch_select_ciq(r.b, nullptr, 0));
    r.calls();
    r.wait();
  }
  { // the same on the in-order schedule (C = 64: split_post; concurrency 0: the caller's stream)
    for (int conc = 0; conc < 3; conc += 2)
    {
      Run r(nm("io C=64 concurrency=%d all outputs, selections", conc), kRef, 64, conc);
      r.feed_on(2);
      r.want_mpx = FMD_MPX_S16;
      r.want_feed = FMD_FEED_F32;
      r.want_ciq = FMD_CIQ_S16;
      const unsigned a[2] = {63, 0};
      OK(fmd_batch_select_audio(r.b, a, 2));
      OK(fmd_batch_select_mpx(r.b, a, 2));
      OK(fmd_batch_select_feed(r.b, a, 1));
      OK(fmd_batch_select_ciq(r.b, a, 2));
      r.calls();
      r.wait();
    }
  }
  for (int mode = 1; mode <= 2; mode++)
    for (unsigned C : {64u, 192u})
    {
      Run r(nm("io C=%u set_rds_blocks %d", C, mode), kRef, C, 2);
      OK(fmd_batch_set_rds_blocks(r.b, mode, 0));
      r.calls();
      fmd_rds_block out[16];
      unsigned lost = 0;
      OK(fmd_batch_collect_rds_blocks(r.b, out, 16, 0, nullptr, &lost));
      r.wait();
    }
  for (unsigned C : {2u, 192u})
  { // the host-buffer call
    Run r(nm("io C=%u host-buffer calls", C), kRef, C, -1);
    r.feed_on(2);
    for (unsigned n : kSizes)
    {
      printf("-- call %u samples\n", n);
      fmd_call c = r.record(n);
      c.mpx = {r.mpx, FMD_MPX_F32, r.sm, nullptr};
      c.feed = {r.feed, FMD_FEED_S16, r.sf, nullptr};
      c.ciq = {r.ciq, FMD_CIQ_F32, r.sm, nullptr};
      OK(fmd_batch_process_host_call(r.b, &c));
    }
    float ms[4];
    OK(fmd_batch_debug_host_ms(r.b, ms));
  }
}

void edits()
{
  for (unsigned C : {192u, 8200u})
  {
    Run r(nm("edits C=%u capture map, switch_captures", C), kRef, C, 2);
    std::vector<unsigned> map(C);
    for (unsigned c = 0; c < C; c++)
      map[c] = (c * 7) % 3;
    OK(fmd_batch_set_capture_map(r.b, map.data(), 3));
    r.iq_stride = 65536;
    r.calls(kSizes, 3);
    const unsigned ch[3] = {1, 100, C - 1}, cap[3] = {2, 0, 1};
    OK(fmd_batch_switch_captures(r.b, ch, cap, 3));
    r.calls(kSizes + 1, 3);
    r.wait();
  }
  for (unsigned C : {192u, 8200u})
  {
    Run r(nm("edits C=%u enable_retune, retune_channels", C), kRef, C, 2);
    OK(fmd_batch_enable_retune(r.b));
    r.calls(kSizes, 3);
    const unsigned ch[2] = {3, C - 2};
    const int sh[2] = {5, -9};
    OK(fmd_batch_retune_channels(r.b, ch, sh, 2));
    r.calls(kSizes + 1, 3);
    r.wait();
  }
  for (unsigned C : {64u, 192u, 8192u})
  {
    Run r(nm("edits C=%u reset_channels", C), kRef, C, 2);
    r.calls(kSizes, 3);
    const unsigned ch[2] = {0, C - 1};
    OK(fmd_batch_reset_channels(r.b, ch, 2));
    r.calls(kSizes + 1, 3); // (the _org ring kernels from here on)
    if (C == 192)
    {
      r.scenario("edits C=192 reset_channels, then ring4=0");
      r.key("ring4", 0);
      r.calls();
    }
    r.wait();
  }
  {
    Run r("edits C=192 export_channels, import_channels, save_state, load_state", kRef, 192, 2);
    r.calls(kSizes, 3);
    const unsigned ch[2] = {7, 150}, to[2] = {8, 9};
    std::vector<char> blob(fmd_batch_state_size(r.b, 2));
    size_t got = 0;
    OK(fmd_batch_export_channels(r.b, ch, 2, blob.data(), blob.size(), &got));
    OK(fmd_batch_import_channels(r.b, to, 2, blob.data(), got));
    r.calls(kSizes + 1, 3);
    std::vector<char> all(fmd_batch_state_size(r.b, 192));
    OK(fmd_batch_save_state(r.b, all.data(), all.size(), &got));
    OK(fmd_batch_load_state(r.b, all.data(), got));
    r.calls(kSizes, 4);
    r.wait();
  }
}

void busy_caller()
{
  for (unsigned C : {64u, 192u})
    for (int conc = 1; conc <= 2; conc++)
    {
      Run r(nm("caller's stream busy C=%u concurrency=%d", C, conc), kRef, C, conc);
      r.stream = rec_stream();
      rec_busy(1);
      r.calls();
      rec_busy(0);
      r.wait();
    }
}

void short_calls()
{
  for (unsigned C : {64u, 192u})
  {
    Run r(nm("short calls C=%u", C), kRef, C, 2);
    const unsigned m = fmd_batch_min_samples(r.b);
    const unsigned sizes[6] = {m, 65536, m + 11, m, 3 * m, m};
    r.calls(sizes, 6);
    r.wait();
  }
  {
    Run r("short calls C=8192", kRef, 8192, 2);
    const unsigned m = fmd_batch_min_samples(r.b);
    const unsigned sizes[4] = {65536, m, 4 * m, m};
    r.calls(sizes, 4);
    r.wait();
  }
}

void other_geometries()
{
  for (unsigned C : {192u, 1024u})
  { // a long IF filter: layout 0 by default, 256-output tiles
    Run r(nm("geometry 2.4 MS/s / 11, 1000 taps, C=%u", C), geometry(2.4e6, 11, 1000), C, 2);
    r.calls();
    r.wait();
  }
  {
    Run r("geometry 400 kS/s / 1: 11-tap first stage, C=192", geometry(400e3, 1), 192, 2, 32768);
    const unsigned sizes[4] = {32000, 32001, 20000, 8193};
    r.calls(sizes, 4);
    r.wait();
  }
  {
    Run r("geometry 6.4 MS/s / 1: CIC first stage, C=192", geometry(6.4e6, 1), 192, 2, 32768);
    const unsigned sizes[4] = {32000, 20000, 4000, 2048};
    r.calls(sizes, 4);
    r.wait();
  }
  const struct
  {
    double fs;
    unsigned D;
  } more[] = {{1.2e6, 5}, {2.048e6, 9}, {1.92e6, 8}, {1.0e6, 4}};
  for (const auto& g : more)
  {
    Run r(nm("geometry %.0f S/s / %u, C=256 concurrency=1 halfband_chain=1", g.fs, g.D), geometry(g.fs, g.D), 256, 1);
    r.key("halfband_chain", 1);
    r.calls();
    r.wait();
  }
}
/* one line per state blob: its size and a 64-bit FNV-1a of its bytes (the header carries the state table's
 * fingerprint, the payload every region's bytes: rows, element sizes, offsets and groups of the table are pinned) */
void blob_line(const char* what, const void* p, size_t n)
{
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; i++)
    h = (h ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
  printf("blob %s %zu bytes fnv1a %016llx\n", what, n, static_cast<unsigned long long>(h));
}

/* The host code around the call path: the walk over a batch's parts (a plain batch, C = 192; a shell over two
 * sub-batches, C = 8200), the record queues' drains, the carried regions of save / load / export / import and of a
 * retune, and the settings a shell mirrors into its sub-batches. */
void parts_regions_queues()
{
  {
    Run r("parts C=8200 set_rds_blocks 2, collect_rds_blocks lag 0 and 2", kRef, 8200, 2);
    OK(fmd_batch_set_rds_blocks(r.b, 2, 0));
    r.calls(kSizes, 3);
    std::vector<fmd_rds_block> out(64);
    unsigned lost = 0;
    OK(fmd_batch_collect_rds_blocks(r.b, out.data(), 64, 0, nullptr, &lost));
    r.calls(kSizes + 1, 3);
    OK(fmd_batch_collect_rds_blocks(r.b, out.data(), 64, 2, nullptr, &lost));
    r.call(kSizes[0]);
    OK(fmd_batch_collect_rds_blocks(r.b, out.data(), 64, 0, nullptr, &lost));
    r.call(kSizes[1]);
    r.wait();
  }
  for (unsigned C : {192u, 8200u})
    for (int lag : {0, 2})
    {
      {
        Run r(nm("parts C=%u collect_rds_lagged lag %d", C, lag), kRef, C, 2);
        r.calls(kSizes, 3);
        std::vector<fmd_rds_group> out(64);
        OK(fmd_batch_collect_rds_lagged(r.b, out.data(), 64, 1, lag, nullptr));
        r.call(kSizes[3]);
        OK(fmd_batch_collect_rds_lagged(r.b, out.data(), 64, 0, lag, nullptr)); // (the slots the first one left)
        r.call(kSizes[0]);
        r.wait();
      }
      {
        Run r(nm("parts C=%u export_rds_device lag %d", C, lag), kRef, C, 2);
        const unsigned cap = 256;
        void* d_records = rows(size_t(cap) * 16); // (real memory: the double's hipMemsetAsync writes it)
        r.calls(kSizes, 3);
        OK(fmd_batch_export_rds_device(r.b, static_cast<int32_t*>(d_records), cap, 1000, lag, nullptr));
        r.call(kSizes[3]);
        r.scenario(nm("parts C=%u export_rds_device lag %d, the drained slots come round again", C, lag));
        rec_busy(1); // (the drained events have not completed: the calls that reuse the slots wait for them)
        for (int i = 0; i < 8; i++)
          r.call(kSizes[i % 4]);
        rec_busy(0);
        OK(fmd_batch_export_rds_device(r.b, static_cast<int32_t*>(d_records), cap, 0, lag, nullptr));
        r.call(kSizes[1]);
        r.wait();
        free(d_records);
      }
    }
  for (unsigned C : {8200u, 192u})
  { // channels on both sides of the sub-batch border (C = 8200: 4224 + 3976); C = 192: with a retune in front
    Run r(nm("parts C=%u export_channels, import_channels, save_state, load_state%s", C,
             C == 192 ? " behind a retune" : ""),
          kRef, C, 2);
    if (C == 192)
      OK(fmd_batch_enable_retune(r.b));
    r.calls(kSizes, 3);
    if (C == 192)
    {
      const unsigned ch[2] = {3, 190};
      const int sh[2] = {5, -9};
      OK(fmd_batch_retune_channels(r.b, ch, sh, 2));
      r.calls(kSizes + 1, 2);
    }
    const unsigned ch[4] = {C - 1, 7, C / 2 + 200 < C ? C / 2 + 200 : 100, C / 2 - 50};
    const unsigned to[4] = {8, C - 2, 9, C / 2 + 30};
    std::vector<char> blob(fmd_batch_state_size(r.b, 4));
    size_t got = 0, all_n = 0;
    OK(fmd_batch_export_channels(r.b, ch, 4, blob.data(), blob.size(), &got));
    blob_line("export_channels", blob.data(), got);
    OK(fmd_batch_import_channels(r.b, to, 4, blob.data(), got));
    r.calls(kSizes + 1, 3);
    std::vector<char> all(fmd_batch_state_size(r.b, C));
    OK(fmd_batch_save_state(r.b, all.data(), all.size(), &all_n));
    blob_line("save_state", all.data(), all_n);
    OK(fmd_batch_load_state(r.b, all.data(), all_n));
    r.calls(kSizes, 2);
    r.scenario(nm("parts C=%u debug_state_skip 4, import and load again", C));
    OK(fmd_batch_debug_state_skip(r.b, 4));
    OK(fmd_batch_export_channels(r.b, ch, 4, blob.data(), blob.size(), &got)); // (a blob of the batch's clock)
    OK(fmd_batch_import_channels(r.b, to, 4, blob.data(), got));
    r.calls(kSizes, 2);
    OK(fmd_batch_load_state(r.b, all.data(), all_n));
    r.calls(kSizes + 2, 2);
    OK(fmd_batch_save_state(r.b, all.data(), all.size(), &all_n));
    blob_line("save_state behind the skipped load", all.data(), all_n);
    r.wait();
  }
  { // every setter that mirrors a setting into the sub-batches; two calls behind each
    Run r("parts C=8200 set_debug_taps", kRef, 8200, 2);
    OK(fmd_batch_enable_retune(r.b));
    r.calls(kSizes, 2);
    OK(fmd_batch_set_debug_taps(r.b, 1));
    r.calls(kSizes, 2);
    r.scenario("parts C=8200 set_profiling 1");
    OK(fmd_batch_set_profiling(r.b, 1));
    r.calls(kSizes + 1, 2);
    float ms[32];
    OK(fmd_batch_get_stage_ms(r.b, ms, 32));
    OK(fmd_batch_set_profiling(r.b, 0));
    r.scenario("parts C=8200 set_channels_per_capture 8");
    OK(fmd_batch_set_channels_per_capture(r.b, 8));
    r.iq_stride = 65536;
    r.calls(kSizes + 2, 2);
    OK(fmd_batch_set_channels_per_capture(r.b, 1));
    r.iq_stride = 0;
    r.scenario("parts C=8200 debug_restart_skip 2, retunes on both sides of the border");
    OK(fmd_batch_debug_restart_skip(r.b, 2));
    const unsigned ch[3] = {1, 4300, 8199};
    const int sh[3] = {5, -9, 2};
    OK(fmd_batch_retune_channels(r.b, ch, sh, 3));
    r.calls(kSizes, 2);
    OK(fmd_batch_debug_restart_skip(r.b, -1));
    r.scenario("parts C=8200 debug_state_skip 1, an import on both sides of the border");
    std::vector<char> blob(fmd_batch_state_size(r.b, 3));
    size_t got = 0;
    OK(fmd_batch_export_channels(r.b, ch, 3, blob.data(), blob.size(), &got));
    blob_line("export_channels", blob.data(), got);
    OK(fmd_batch_debug_state_skip(r.b, 1));
    OK(fmd_batch_import_channels(r.b, ch, 3, blob.data(), got));
    r.calls(kSizes + 1, 2);
    OK(fmd_batch_debug_state_skip(r.b, -1));
    r.scenario("parts C=8200 debug_reset_keep_ring_phase 1, resets on both sides of the border");
    OK(fmd_batch_debug_reset_keep_ring_phase(r.b, 1));
    OK(fmd_batch_reset_channels(r.b, ch, 3));
    r.calls(kSizes + 2, 2);
    r.wait();
  }
}
} // namespace

int main()
{
  setvbuf(stdout, nullptr, _IOFBF, 1 << 16);
  printf("== kernels\n");
  rec_kernels();
  basic_modes();
  layouts();
  chain_and_ring_small();
  large_batch();
  sub_batches();
  inputs_and_outputs();
  edits();
  busy_caller();
  short_calls();
  other_geometries();
  parts_regions_queues();
  return 0;
}
