/*
 * ciq_in_trace.cpp -- the driver of tests/test_ciq_in_trace_cpu.py: process calls with IQ and with channel IQ rows as
 * their input (FMD_IN_CIQ_*) through the C ABI of include/fmd.h, linked against the recording double of the HIP
 * runtime (tests/cpp/call_trace/hip_recorder.cpp) with the host objects fmd_batch.o and fmd_ciq_in.o.  It prints a
 * "== name" line per scenario and every runtime call the library made, with a "-- call <kind> <length>" line in front of
 * every process call.  No kernel runs and no GPU is opened.
 */
#include "fmd.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>

extern "C" void rec_on(int);
extern "C" void rec_epoch();

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

void* rows(size_t bytes)
{
  void* p = nullptr;
  if (posix_memalign(&p, 64, bytes))
    die("posix_memalign", -1);
  return p;
}

/* IQ, float rows, int16 rows, IQ: every call of baseband length 5958 or 5957 (65 536 samples at D = 11) */
void scenario(const char* name, unsigned C, int conc, int profiling)
{
  fmd_params p{};
  p.sample_rate_if = 2.4e6;
  p.tuning_offset = -0.15 * 2.4e6;
  p.sample_rate_pcm = 48000.0;
  p.bandwidth_pcm = 15000.0;
  p.downsample = 11;
  printf("== %s\n", name);
  rec_epoch();
  rec_on(1);
  fmd_batch* b = nullptr;
  OK(fmd_batch_create(&p, C, nullptr, 0, nullptr, nullptr, &b));
  OK(fmd_batch_set_concurrency(b, conc));
  if (profiling)
    OK(fmd_batch_set_profiling(b, profiling));
  const size_t sa = (fmd_batch_max_audio_floats(b, 65536) + 15) / 16 * 16, sq = 5968;
  void* iq = rows(size_t(65536) * 8);
  void* ciq = rows(sq * C * 8);
  void* audio = rows(sa * C * 4);
  const struct
  {
    const char* kind;
    int fmt;
    unsigned n;
  } calls[] = {{"iq", FMD_IQ_F32, 65536}, {"ciq_f32", FMD_IN_CIQ_F32, 5958}, {"ciq_s16", FMD_IN_CIQ_S16, 5958},
               {"iq", FMD_IQ_F32, 65536}};
  for (const auto& k : calls)
  {
    printf("-- call %s %u\n", k.kind, k.n);
    fmd_call c{};
    c.size = sizeof(c);
    c.iq = k.fmt == FMD_IQ_F32 ? iq : ciq;
    c.iq_format = k.fmt;
    c.iq_channel_stride = k.fmt == FMD_IQ_F32 ? 0 : sq;
    c.samples = k.n;
    c.audio = {audio, FMD_PCM_F32, sa, nullptr};
    OK(fmd_batch_process_device_call(b, &c));
  }
  printf("-- end\n");
  OK(fmd_batch_wait(b, nullptr));
  fmd_batch_destroy(b);
  rec_on(0);
  free(iq);
  free(ciq);
  free(audio);
}
} // namespace

int main()
{
  scenario("C=192 concurrency 2", 192, 2, 0);
  scenario("C=192 concurrency 0", 192, 0, 0);
  scenario("C=192 concurrency 1 profiling 1", 192, 1, 1);
  scenario("C=192 profiling 2", 192, 2, 2);
  scenario("C=1024 concurrency 2", 1024, 2, 0);
  return 0;
}
