/*
 * fmd_scan.inc.hpp -- the band scan's host side (fmd_scan_*, include/fmd.h): parameter checks, the window, twiddle
 * and slot tables, and the launches of csrc/fmd_k_scan.hip.h on the caller's stream.  Included by fmd_batch.hip
 * (one translation unit: it shares g_err / fail / HIPCHK).  A scan owns no stream and no state of any fmd_batch.
 */
struct fmd_scan
{
  int device = 0;
  unsigned G = 0, N = 0, T = 0, floor_index = 0;
  double fs = 0.0, sum_w2 = 0.0;
  float threshold_db = 0.0f;
  unsigned long long segments = 0; // K: segments accumulated since the last reset (host count, call order)
  DevBuf<float> d_win;
  DevBuf<float2> d_tw;
  DevBuf<double> d_totals;
  DevBuf<fmd::ScanSlot> d_slots;
  DevBuf<float> d_scratch;
  DevBuf<char> d_stage; // fmd_scan_accumulate_host / fmd_scan_finish_host

  ~fmd_scan() { (void)hipSetDevice(device); } // (the buffers free themselves behind it)
};

namespace
{

/* Few captures: below this count each capture's chunks are spread over workgroups (scratch + k_scan_reduce). */
constexpr unsigned kScanSplitBelow = 512;

template <class In, int N>
void scan_launch(fmd_scan* s, const void* d_iq, size_t stride, unsigned S, unsigned n_chunks, hipStream_t stream)
{
  const auto* x = static_cast<const typename In::elem*>(d_iq);
  if (s->d_scratch.p && s->G < kScanSplitBelow)
  {
    hipLaunchKernelGGL((fmd::k_scan_psd<In, N>), dim3(n_chunks, s->G), dim3(fmd::kScanThreads), 0, stream, x,
                       stride, S, n_chunks, s->d_win.p, s->d_tw.p, s->d_totals.p, s->d_scratch.p);
    const size_t n = size_t(s->G) * N;
    hipLaunchKernelGGL(fmd::k_scan_reduce, dim3(unsigned((n + 255) / 256)), dim3(256), 0, stream, s->d_totals.p,
                       s->d_scratch.p, s->G, unsigned(N), n_chunks);
  }
  else
    hipLaunchKernelGGL((fmd::k_scan_psd<In, N>), dim3(s->G), dim3(fmd::kScanThreads), 0, stream, x, stride, S,
                       n_chunks, s->d_win.p, s->d_tw.p, s->d_totals.p, static_cast<float*>(nullptr));
}

template <class In>
void scan_launch_n(fmd_scan* s, const void* d_iq, size_t stride, unsigned S, unsigned n_chunks, hipStream_t stream)
{
  switch (s->N)
  {
  case 256: scan_launch<In, 256>(s, d_iq, stride, S, n_chunks, stream); break;
  case 512: scan_launch<In, 512>(s, d_iq, stride, S, n_chunks, stream); break;
  case 1024: scan_launch<In, 1024>(s, d_iq, stride, S, n_chunks, stream); break;
  case 2048: scan_launch<In, 2048>(s, d_iq, stride, S, n_chunks, stream); break;
  default: scan_launch<In, 4096>(s, d_iq, stride, S, n_chunks, stream); break;
  }
}

int scan_accumulate(fmd_scan* s, const void* d_iq, IqFormat fmt, size_t stride, unsigned samples, void* stream_)
{
  if (!s || !d_iq)
    return fail(FMD_ERR_ARG, "fmd_scan_accumulate: null scan or IQ pointer");
  const size_t pair = 2 * format_esz(FMT_IQ, fmt);
  if (reinterpret_cast<uintptr_t>(d_iq) % pair || (s->G > 1 && stride % 2))
    return fail(FMD_ERR_ARG, "fmd_scan_accumulate: IQ pointer and capture stride must be multiples of two IQ samples");
  if (s->G > 1 && stride < samples)
    return fail(FMD_ERR_ARG, "fmd_scan_accumulate: the capture stride is shorter than a capture (samples)");
  if (samples < s->N)
    return fail(FMD_ERR_SIZE, "fmd_scan_accumulate: fewer samples than one segment (nfft)");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK(hipSetDevice(s->device));
  const unsigned S = (samples - s->N) / (s->N / 2) + 1;
  const unsigned n_chunks = (S + fmd::kScanChunk - 1) / fmd::kScanChunk;
  const size_t scratch = size_t(s->G) * n_chunks * s->N;
  if (s->G < kScanSplitBelow && scratch > s->d_scratch.n)
  {
    HIPCHK(hipStreamSynchronize(stream)); // the old buffer may still be read by work queued on this stream
    if (s->d_scratch.alloc(scratch))
      return fail(FMD_ERR_DEVICE, "fmd_scan: device allocation failed");
    // alloc() zero-fills on the null stream, which a non-blocking caller's stream is not ordered behind: without
    // this the fill could land on partials the kernels below have already written
    HIPCHK(hipStreamSynchronize(nullptr));
  }
  switch (fmt)
  {
  case IQ_U8: scan_launch_n<fmd::InU8>(s, d_iq, stride, S, n_chunks, stream); break;
  case IQ_S8: scan_launch_n<fmd::InS8>(s, d_iq, stride, S, n_chunks, stream); break;
  case IQ_S16: scan_launch_n<fmd::InS16>(s, d_iq, stride, S, n_chunks, stream); break;
  default: scan_launch_n<fmd::InF32>(s, d_iq, stride, S, n_chunks, stream); break;
  }
  HIPCHK(hipGetLastError());
  s->segments += S;
  return FMD_OK;
}

int scan_finish(fmd_scan* s, float* d_psd, float* d_slot_db, float* d_floor_db, fmd_scan_candidate* d_cand,
                unsigned max_cand, uint32_t* d_counts, hipStream_t stream)
{
  if (s->segments == 0)
    return fail(FMD_ERR_STATE, "fmd_scan_finish: no segment has been accumulated since the last reset");
  HIPCHK(hipSetDevice(s->device));
  fmd::ScanSlotArgs a{};
  a.totals = s->d_totals.p;
  a.slots = s->d_slots.p;
  a.denom = double(s->segments) * double(s->N) * s->sum_w2;
  a.N = s->N;
  a.T = s->T;
  a.floor_index = s->floor_index;
  a.max_cand = d_cand ? max_cand : 0u;
  a.threshold_db = s->threshold_db;
  a.psd = d_psd;
  a.slot_db = d_slot_db;
  a.floor_db = d_floor_db;
  a.cand = reinterpret_cast<fmd::ScanCandidate*>(d_cand);
  a.counts = d_counts;
  hipLaunchKernelGGL(fmd::k_scan_slots, dim3(s->G), dim3(256), 0, stream, a);
  HIPCHK(hipGetLastError());
  return FMD_OK;
}

} // namespace

static_assert(sizeof(fmd_scan_candidate) == sizeof(fmd::ScanCandidate), "candidate layout");

extern "C" {

int fmd_scan_create(const fmd_scan_params* p, unsigned n_captures, int device, fmd_scan** out)
{
  if (!p || !out)
    return fail(FMD_ERR_ARG, "fmd_scan_create: null argument");
  *out = nullptr;
  if (n_captures == 0)
    return fail(FMD_ERR_ARG, "fmd_scan_create: zero captures");
  const unsigned N = p->nfft ? p->nfft : 1024u;
  const unsigned T = p->table_size ? p->table_size : 64u;
  const double hw = p->half_width_hz != 0.0 ? p->half_width_hz : 100e3;
  const double sep = p->min_separation_hz != 0.0 ? p->min_separation_hz : 150e3;
  const float thr = p->threshold_db != 0.0f ? p->threshold_db : 10.0f;
  const float qf = p->floor_quantile != 0.0f ? p->floor_quantile : 0.2f;
  const double fs = p->sample_rate_if;
  if (!(fs > 0.0) || !std::isfinite(fs))
    return fail(FMD_ERR_ARG, "fmd_scan_create: sample_rate_if must be a positive rate");
  if (N < 256 || N > unsigned(fmd::kScanMaxN) || (N & (N - 1)))
    return fail(FMD_ERR_ARG, "fmd_scan_create: nfft must be a power of two from 256 to 4096");
  if (T > unsigned(fmd::kScanMaxSlots))
    return fail(FMD_ERR_ARG, "fmd_scan_create: table_size above 1024 slots is not supported by the scan");
  if (!(hw > 0.0) || !std::isfinite(hw) || !(sep >= 0.0) || !std::isfinite(sep))
    return fail(FMD_ERR_ARG, "fmd_scan_create: half_width_hz must be positive and min_separation_hz not negative");
  if (!(qf > 0.0f && qf < 1.0f))
    return fail(FMD_ERR_ARG, "fmd_scan_create: floor_quantile must lie strictly between 0 and 1");
  if (!std::isfinite(thr))
    return fail(FMD_ERR_ARG, "fmd_scan_create: threshold_db must be finite");

  // tables (host, double): window, twiddles, slots
  std::vector<float> win(N);
  std::vector<float2> tw(N);
  double sw2 = 0.0;
  for (unsigned n = 0; n < N; ++n)
  {
    const double w = 0.5 - 0.5 * std::cos(2.0 * M_PI * double(n) / double(N));
    win[n] = float(w);
    sw2 += double(win[n]) * double(win[n]);
    const double a = -2.0 * M_PI * double(n) / double(N);
    tw[n] = make_float2(float(std::cos(a)), float(std::sin(a)));
  }
  const int first = -int(T / 2);
  std::vector<fmd::ScanSlot> slots(T);
  std::vector<double> f(T);
  for (unsigned j = 0; j < T; ++j)
    f[j] = double(-(first + int(j))) * fs / double(T);
  for (unsigned j = 0; j < T; ++j)
  {
    fmd::ScanSlot& s = slots[j];
    s.shift = first + int(j);
    s.offset_hz = float(f[j]);
    s.eligible = std::fabs(f[j]) + hw <= fs / 2.0;
    s.blo = int(N);
    s.bhi = -1;
    for (unsigned i = 0; i < N; ++i)
      if (std::fabs((double(i) - double(N / 2)) * fs / double(N) - f[j]) <= hw)
      {
        s.blo = std::min(s.blo, int(i));
        s.bhi = std::max(s.bhi, int(i));
      }
    if (s.bhi < s.blo)
      s.eligible = 0; // narrower than a bin: nothing to sum
    s.nlo = int(j);
    s.nhi = int(j);
    for (unsigned k = 0; k < T; ++k)
      if (std::fabs(f[k] - f[j]) <= sep)
      {
        s.nlo = std::min(s.nlo, int(k));
        s.nhi = std::max(s.nhi, int(k));
      }
  }

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(FMD_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= ndev)
    return fail(FMD_ERR_ARG, "fmd_scan_create: device ordinal out of range");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<fmd_scan> s(new fmd_scan);
  s->device = device;
  s->G = n_captures;
  s->N = N;
  s->T = T;
  s->fs = fs;
  s->sum_w2 = sw2;
  s->threshold_db = thr;
  s->floor_index = unsigned(std::floor(double(qf) * double(N - 1)));
  // (zero-filled: no segment accumulated yet)
  if (s->d_win.alloc(N) || s->d_tw.alloc(N) || s->d_totals.alloc(size_t(n_captures) * N) || s->d_slots.alloc(T))
    return fail(FMD_ERR_DEVICE, "fmd_scan_create: device allocation failed");
  HIPCHK(hipMemcpy(s->d_win.p, win.data(), N * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(s->d_tw.p, tw.data(), N * sizeof(float2), hipMemcpyHostToDevice));
  if (T)
    HIPCHK(hipMemcpy(s->d_slots.p, slots.data(), T * sizeof(fmd::ScanSlot), hipMemcpyHostToDevice));
  HIPCHK(hipDeviceSynchronize());
  *out = s.release();
  return FMD_OK;
}

void fmd_scan_destroy(fmd_scan* s)
{
  if (s)
    (void)hipDeviceSynchronize();
  delete s;
}

int fmd_scan_reset(fmd_scan* s, void* stream)
{
  if (!s)
    return fail(FMD_ERR_ARG, "fmd_scan_reset: null scan");
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipMemsetAsync(s->d_totals.p, 0, size_t(s->G) * s->N * sizeof(double), static_cast<hipStream_t>(stream)));
  s->segments = 0;
  return FMD_OK;
}

int fmd_scan_slots(const fmd_scan* s, int32_t* first_shift)
{
  if (!s)
    return fail(FMD_ERR_ARG, "fmd_scan_slots: null scan");
  if (first_shift)
    *first_shift = -int32_t(s->T / 2);
  return int(s->T);
}

int fmd_scan_accumulate_device_fmt(fmd_scan* s, const void* d_iq, int format, size_t iq_capture_stride,
                                   unsigned samples, void* stream)
{
  if (!format_ok(FMT_IQ, format))
    return fail(FMD_ERR_ARG, "fmd_scan_accumulate_device_fmt: format must be one of FMD_IQ_F32, _U8, _S8, _S16 (0..3)");
  return scan_accumulate(s, d_iq, IqFormat(format), iq_capture_stride, samples, stream);
}

int fmd_scan_accumulate_device(fmd_scan* s, const float* d_iq, size_t iq_capture_stride, unsigned samples,
                               void* stream)
{
  return fmd_scan_accumulate_device_fmt(s, d_iq, FMD_IQ_F32, iq_capture_stride, samples, stream);
}

int fmd_scan_accumulate_device_u8(fmd_scan* s, const uint8_t* d_iq_u8, size_t iq_capture_stride, unsigned samples,
                                  void* stream)
{
  return fmd_scan_accumulate_device_fmt(s, d_iq_u8, FMD_IQ_U8, iq_capture_stride, samples, stream);
}

int fmd_scan_accumulate_host(fmd_scan* s, const float* iq, size_t iq_capture_stride, unsigned samples)
{
  return fmd_scan_accumulate_host_fmt(s, iq, FMD_IQ_F32, iq_capture_stride, samples);
}

int fmd_scan_accumulate_host_fmt(fmd_scan* s, const void* iq, int format, size_t iq_capture_stride, unsigned samples)
{
  if (!format_ok(FMT_IQ, format))
    return fail(FMD_ERR_ARG, "fmd_scan_accumulate_host_fmt: format must be one of FMD_IQ_F32, _U8, _S8, _S16 (0..3)");
  const IqFormat fmt = IqFormat(format);
  if (!s || !iq)
    return fail(FMD_ERR_ARG, "fmd_scan_accumulate_host: null scan or IQ pointer");
  if (s->G > 1 && iq_capture_stride < samples)
    return fail(FMD_ERR_ARG, "fmd_scan_accumulate_host: the capture stride is shorter than a capture (samples)");
  if (s->G > 1 && iq_capture_stride % 2)
    return fail(FMD_ERR_ARG, "fmd_scan_accumulate_host: the capture stride must be a multiple of two IQ samples");
  if (samples < s->N)
    return fail(FMD_ERR_SIZE, "fmd_scan_accumulate_host: fewer samples than one segment (nfft)");
  HIPCHK(hipSetDevice(s->device));
  const size_t stride = s->G > 1 ? iq_capture_stride : 0;
  const size_t bytes = (size_t(s->G - 1) * stride + samples) * format_esz(FMT_IQ, fmt);
  if (bytes > s->d_stage.n)
  {
    HIPCHK(hipStreamSynchronize(nullptr)); // the old buffer may still be read by work queued on this stream
    if (s->d_stage.alloc(bytes))
      return fail(FMD_ERR_DEVICE, "fmd_scan: device allocation failed");
  }
  HIPCHK(hipMemcpy(s->d_stage.p, iq, bytes, hipMemcpyHostToDevice));
  if (int rc = scan_accumulate(s, s->d_stage.p, fmt, stride, samples, nullptr))
    return rc;
  HIPCHK(hipStreamSynchronize(nullptr));
  return FMD_OK;
}

int fmd_scan_finish_device(fmd_scan* s, float* d_psd, float* d_slot_db, float* d_floor_db, fmd_scan_candidate* d_cand,
                           unsigned max_cand, uint32_t* d_counts, void* stream)
{
  if (!s)
    return fail(FMD_ERR_ARG, "fmd_scan_finish_device: null scan");
  return scan_finish(s, d_psd, d_slot_db, d_floor_db, d_cand, max_cand, d_counts, static_cast<hipStream_t>(stream));
}

int fmd_scan_finish_host(fmd_scan* s, float* psd, float* slot_db, float* floor_db, fmd_scan_candidate* cand,
                         unsigned max_cand, uint32_t* counts)
{
  if (!s)
    return fail(FMD_ERR_ARG, "fmd_scan_finish_host: null scan");
  HIPCHK(hipSetDevice(s->device));
  const size_t G = s->G;
  const size_t n_psd = psd ? G * s->N * sizeof(float) : 0, n_slot = slot_db ? G * s->T * sizeof(float) : 0,
               n_floor = floor_db ? G * sizeof(float) : 0,
               n_cand = (cand && max_cand) ? G * max_cand * sizeof(fmd_scan_candidate) : 0,
               n_counts = counts ? G * sizeof(uint32_t) : 0;
  const size_t o_slot = (n_psd + 15) & ~size_t(15), o_floor = (o_slot + n_slot + 15) & ~size_t(15),
               o_cand = (o_floor + n_floor + 15) & ~size_t(15), o_counts = (o_cand + n_cand + 15) & ~size_t(15),
               total = std::max<size_t>(16, o_counts + n_counts);
  if (total > s->d_stage.n)
  {
    HIPCHK(hipStreamSynchronize(nullptr)); // the old buffer may still be read by work queued on this stream
    if (s->d_stage.alloc(total))
      return fail(FMD_ERR_DEVICE, "fmd_scan: device allocation failed");
  }
  char* base = s->d_stage.p;
  if (int rc = scan_finish(s, psd ? reinterpret_cast<float*>(base) : nullptr,
                           slot_db ? reinterpret_cast<float*>(base + o_slot) : nullptr,
                           floor_db ? reinterpret_cast<float*>(base + o_floor) : nullptr,
                           n_cand ? reinterpret_cast<fmd_scan_candidate*>(base + o_cand) : nullptr, max_cand,
                           counts ? reinterpret_cast<uint32_t*>(base + o_counts) : nullptr, nullptr))
    return rc;
  HIPCHK(hipStreamSynchronize(nullptr));
  if (psd)
    HIPCHK(hipMemcpy(psd, base, n_psd, hipMemcpyDeviceToHost));
  if (slot_db)
    HIPCHK(hipMemcpy(slot_db, base + o_slot, n_slot, hipMemcpyDeviceToHost));
  if (floor_db)
    HIPCHK(hipMemcpy(floor_db, base + o_floor, n_floor, hipMemcpyDeviceToHost));
  if (n_cand)
    HIPCHK(hipMemcpy(cand, base + o_cand, n_cand, hipMemcpyDeviceToHost));
  if (counts)
    HIPCHK(hipMemcpy(counts, base + o_counts, n_counts, hipMemcpyDeviceToHost));
  return FMD_OK;
}

} // extern "C"
