/*
 * fmd_split.inc.hpp -- the band splitter's host side (fmd_split_*, include/fmd.h): parameter checks, the taps and
 * tuner tables, and the launches of csrc/fmd_k_split.hip.h on the caller's stream.  Included by fmd_batch.hip (one
 * translation unit: it shares g_err / fail / HIPCHK).  A splitter owns no stream and no state of any fmd_batch.
 */
struct fmd_split
{
  int device = 0;
  unsigned G = 0, B = 0;
  bool real = false;                // fmd_split_create_real: FMD_REAL_* input, one float a sample in window and history
  double fs = 0.0;
  float scale = 0.5f;
  fmd::SplitGeom geom{};            // the generic form's tile
  bool compiled = false;            // (R, K) has a compile-time form (TO = kSplitThreads)
  unsigned long long q = 0;         // input samples of every capture since create / reset (host, call order)
  unsigned parity = 0;              // which history buffer the next call reads
  std::vector<float> taps;          // c[0 .. K + 1]
  std::vector<int> shifts;          // [G B], as the next call will use them
  bool shifts_dirty = true;         // the device tables are not those of `shifts`
  DevBuf<float> d_coeff;
  DevBuf<float2> d_hist[2];         // [G][K] raw (converted) history, by call parity
  DevBuf<float> d_rhist[2];         // ... of a real splitter
  DevBuf<float2> d_luts;            // [G B][T]: written by an upload on the calls' stream, behind its last reader
  /* Page-locked staging of one version of the tables: the upload in front of a call reads it when the stream gets
   * there, so it is written again only once `done`, recorded behind that upload, has completed.  A set_shifts never
   * waits: with every version still in flight the pool grows by one. */
  struct Staging
  {
    HostBuf<float2> h;
    Event done;
    bool used = false;
  };
  std::vector<std::unique_ptr<Staging>> pool;
  DevBuf<char> d_stage_in, d_stage_out; // fmd_split_process_host

  ~fmd_split() { (void)hipSetDevice(device); } // (the buffers free themselves behind it)
};

namespace
{

/* (R, K) with a compile-time form of k_split: the headline geometries, K = 8 R */
inline bool split_compiled(unsigned R, unsigned K)
{
  return (R == 4 && K == 32) || (R == 8 && K == 64);
}

/* the geometry of a tile of TO outputs, for this splitter's kind */
inline fmd::SplitGeom split_geom_of(const fmd_split* s, unsigned TO)
{
  return fmd::split_geom(s->geom.R, s->geom.K, s->geom.T, TO, s->real);
}

template <class In>
void split_launch(fmd_split* s, const fmd::SplitArgs& a, unsigned ntiles, unsigned lds, hipStream_t stream)
{
  const dim3 grid(ntiles, s->G), block(fmd::kSplitThreads);
  if (s->compiled && a.g.R == 4)
    hipLaunchKernelGGL((fmd::k_split<In, 4, 32>), grid, block, lds, stream, a);
  else if (s->compiled)
    hipLaunchKernelGGL((fmd::k_split<In, 8, 64>), grid, block, lds, stream, a);
  else
    hipLaunchKernelGGL((fmd::k_split<In, 0, 0>), grid, block, lds, stream, a);
}

template <class In>
void split_roll(fmd_split* s, const void* d_in, size_t stride, unsigned samples, hipStream_t stream)
{
  const unsigned K = s->geom.K;
  hipLaunchKernelGGL((fmd::k_split_roll<In>), dim3((K + 255) / 256, s->G), dim3(256), 0, stream, d_in, stride,
                     samples, s->d_hist[s->parity].p, s->d_hist[s->parity ^ 1u].p, K);
}

/* outputs of a call of n samples behind q samples: the multiples of R in [q, q + n) */
inline unsigned split_count(unsigned long long q, unsigned n, unsigned R, unsigned* pos)
{
  const unsigned p = unsigned((R - q % R) % R);
  if (pos)
    *pos = p;
  return n > p ? (n - p - 1) / R + 1 : 0u;
}

/* the argument checks of a process call that need no device */
int split_check(const char* fn, fmd_split* s, const void* in, int format, size_t in_stride, unsigned samples,
                const void* out, size_t out_stride, bool device_call)
{
  const std::string f(fn);
  const bool real = real_format_ok(format);
  if (!real && !format_ok(FMT_IQ, format))
    return fail(FMD_ERR_ARG, f + ": iq_format must be one of FMD_IQ_F32, _U8, _S8, _S16 (0..3)");
  if (!s || !in || !out)
    return fail(FMD_ERR_ARG, f + ": null splitter, input or output pointer");
  if (real != s->real)
    return fail(FMD_ERR_ARG,
                f + (s->real ? ": this is a real splitter (fmd_split_create_real), iq_format must be one of "
                               "FMD_REAL_F32, _S8, _S16 (16, 18, 19)"
                             : ": this is a complex splitter (fmd_split_create), iq_format must be one of "
                               "FMD_IQ_F32, _U8, _S8, _S16 (0..3)"));
  if (samples == 0 || samples > FMD_SPLIT_MAX_SAMPLES)
    return fail(FMD_ERR_SIZE, f + ": samples must be 1 .. FMD_SPLIT_MAX_SAMPLES (16777216)");
  if (s->G > 1 && in_stride < samples)
    return fail(FMD_ERR_ARG, f + ": in_capture_stride is shorter than a capture (samples)");
  const unsigned M = split_count(s->q, samples, s->geom.R, nullptr);
  if (s->G * s->B > 1 && out_stride < M)
    return fail(FMD_ERR_ARG, f + ": out_row_stride is shorter than the call's output count");
  if (device_call)
  {
    if (real)
    {
      if (reinterpret_cast<uintptr_t>(in) % (4 * real_format_esz(format)) || (s->G > 1 && in_stride % 4))
        return fail(FMD_ERR_ARG, f + ": d_in and in_capture_stride must be multiples of four real samples");
    }
    else
    {
      const size_t pair = 2 * format_esz(FMT_IQ, format);
      if (reinterpret_cast<uintptr_t>(in) % pair || (s->G > 1 && in_stride % 2))
        return fail(FMD_ERR_ARG, f + ": d_in and in_capture_stride must be multiples of two IQ samples");
    }
    if (reinterpret_cast<uintptr_t>(out) % 16 || out_stride % 2)
      return fail(FMD_ERR_ARG, f + ": d_out must be 16-byte aligned and out_row_stride even");
    if (out_stride < M)
      return fail(FMD_ERR_ARG, f + ": out_row_stride is shorter than the call's output count");
  }
  return FMD_OK;
}

/* the tables of s->shifts into d_luts, on the calls' stream in front of the next kernel */
int split_upload_tables(fmd_split* s, hipStream_t stream)
{
  const unsigned T = s->geom.T, rows = s->G * s->B;
  fmd_split::Staging* st = nullptr;
  for (auto& p : s->pool)
    if (!p->used || hipEventQuery(p->done) == hipSuccess)
    {
      st = p.get();
      break;
    }
  if (!st)
  {
    std::unique_ptr<fmd_split::Staging> p(new fmd_split::Staging);
    if (p->h.alloc(size_t(rows) * T) || p->done.create() != hipSuccess)
      return fail(FMD_ERR_DEVICE, "fmd_split: page-locked allocation failed");
    st = p.get();
    s->pool.push_back(std::move(p));
  }
  // (bands of different captures mostly share their shifts: each table is computed once)
  std::map<int, std::vector<float>> by_shift;
  for (unsigned r = 0; r < rows; r++)
  {
    auto it = by_shift.find(s->shifts[r]);
    if (it == by_shift.end())
      it = by_shift.emplace(s->shifts[r], fmd::make_tuner_lut(T, s->shifts[r])).first;
    std::memcpy(st->h.p + size_t(r) * T, it->second.data(), size_t(T) * sizeof(float2));
  }
  HIPCHK(hipMemcpyAsync(s->d_luts.p, st->h.p, size_t(rows) * T * sizeof(float2), hipMemcpyHostToDevice, stream));
  HIPCHK(hipEventRecord(st->done, stream));
  st->used = true;
  s->shifts_dirty = false;
  return FMD_OK;
}

int split_process(fmd_split* s, const void* d_in, int fmt, size_t in_stride, unsigned samples, float2* d_out,
                  size_t out_stride, unsigned* out_samples, hipStream_t stream)
{
  HIPCHK(hipSetDevice(s->device));
  if (s->shifts_dirty)
    if (int rc = split_upload_tables(s, stream))
      return rc;
  const fmd::SplitGeom& g = s->geom;
  fmd::SplitArgs a{};
  a.in = d_in;
  a.in_stride = s->G > 1 ? in_stride : 0;
  a.hist = s->real ? static_cast<const void*>(s->d_rhist[s->parity].p) : s->d_hist[s->parity].p;
  a.luts = s->d_luts.p;
  a.coeff = s->d_coeff.p;
  a.out = d_out;
  a.out_stride = out_stride;
  a.N = samples;
  a.B = s->B;
  a.M = split_count(s->q, samples, g.R, &a.pos);
  a.lut_k = unsigned((s->q % g.T + size_t(g.T) * ((g.K + g.T - 1) / g.T) - g.K) % g.T);
  a.lut_step = unsigned(fmd::kSplitThreads) % g.T;
  a.scale = s->scale;
  a.g = s->compiled ? split_geom_of(s, fmd::kSplitThreads) : g;
  if (a.M)
  {
    const unsigned ntiles = (a.M + a.g.TO - 1) / a.g.TO;
    const unsigned lds = a.g.total * unsigned(sizeof(float2));
    switch (fmt)
    {
    case FMD_REAL_F32:
    case FMD_REAL_S8:
    case FMD_REAL_S16: // (the real forms: fmd_split_real.hip)
      fmd::split_real_launch(fmt, s->compiled ? int(g.R) : 0, ntiles, s->G, lds, stream, a);
      break;
    case IQ_U8: split_launch<fmd::InU8>(s, a, ntiles, lds, stream); break;
    case IQ_S8: split_launch<fmd::InS8>(s, a, ntiles, lds, stream); break;
    case IQ_S16: split_launch<fmd::InS16>(s, a, ntiles, lds, stream); break;
    default: split_launch<fmd::InF32>(s, a, ntiles, lds, stream); break;
    }
  }
  switch (fmt)
  {
  case FMD_REAL_F32:
  case FMD_REAL_S8:
  case FMD_REAL_S16:
    fmd::split_real_roll(fmt, s->G, g.K, d_in, a.in_stride, samples, s->d_rhist[s->parity].p,
                         s->d_rhist[s->parity ^ 1u].p, stream);
    break;
  case IQ_U8: split_roll<fmd::InU8>(s, d_in, a.in_stride, samples, stream); break;
  case IQ_S8: split_roll<fmd::InS8>(s, d_in, a.in_stride, samples, stream); break;
  case IQ_S16: split_roll<fmd::InS16>(s, d_in, a.in_stride, samples, stream); break;
  default: split_roll<fmd::InF32>(s, d_in, a.in_stride, samples, stream); break;
  }
  HIPCHK(hipGetLastError());
  s->parity ^= 1u;
  s->q += samples;
  if (out_samples)
    *out_samples = a.M;
  return FMD_OK;
}

/* fmd_split_create / fmd_split_create_real: the same parameters, ranges and defaults */
int split_create(const char* fn, bool real, const fmd_split_params* p, unsigned n_captures, unsigned n_bands,
                 const int* shifts, int device, fmd_split** out)
{
  const std::string f(fn);
  if (!p || !out || !shifts)
    return fail(FMD_ERR_ARG, f + ": null argument (params, shifts or out)");
  *out = nullptr;
  if (n_captures == 0 || n_captures > 65535u)
    return fail(FMD_ERR_ARG, f + ": n_captures must be 1 .. 65535");
  if (n_bands == 0 || size_t(n_captures) * n_bands > (size_t(1) << 20))
    return fail(FMD_ERR_ARG, f + ": n_bands must be at least 1 and n_captures * n_bands at most 2^20");
  const double fs = p->sample_rate_in;
  if (!(fs > 0.0) || !std::isfinite(fs))
    return fail(FMD_ERR_ARG, f + ": sample_rate_in must be a positive rate");
  const unsigned R = p->decimation;
  if (R < 2 || R > 64)
    return fail(FMD_ERR_ARG, f + ": decimation must be 2 .. 64");
  const unsigned K = p->filter_order ? p->filter_order : 8 * R;
  if (K < 2 || K > 1024)
    return fail(FMD_ERR_ARG, f + ": filter_order must be 2 .. 1024 (0 = 8 * decimation)");
  const double cutoff = p->cutoff != 0.0 ? p->cutoff : 0.6 / double(R);
  if (!(cutoff > 0.0 && cutoff <= 0.5))
    return fail(FMD_ERR_ARG, f + ": cutoff must lie in (0, 0.5] of the input rate (0 = 0.6 / decimation)");
  const unsigned T = p->table_size ? p->table_size : 64u;
  if (T > 1024)
    return fail(FMD_ERR_ARG, f + ": table_size must be 1 .. 1024 (0 = 64)");
  if (!std::isfinite(p->out_scale))
    return fail(FMD_ERR_ARG, f + ": out_scale must be a finite float (0 = 0.5)");
  // the largest tile of outputs whose windows fit the LDS of a workgroup
  unsigned TO = fmd::kSplitThreads;
  while (TO > 1 && fmd::split_geom(R, K, T, TO, real).total * sizeof(float2) > fmd::kSplitLdsBytes)
    TO--;
  const fmd::SplitGeom geom = fmd::split_geom(R, K, T, TO, real);
  if (geom.total * sizeof(float2) > fmd::kSplitLdsBytes)
    return fail(FMD_ERR_ARG, f + ": filter_order and table_size do not fit a workgroup's LDS");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(FMD_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= ndev)
    return fail(FMD_ERR_ARG, f + ": device ordinal out of range");
  if (real && (!fmd::split_real_launch || !fmd::split_real_roll)) // (never in the library: fmd_k_split.hip.h)
    return fail(FMD_ERR_DEVICE, f + ": the real forms' kernels (fmd_split_real.o) are not linked into this program");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<fmd_split> s(new fmd_split);
  s->device = device;
  s->real = real;
  s->G = n_captures;
  s->B = n_bands;
  s->fs = fs;
  s->scale = p->out_scale != 0.0f ? p->out_scale : 0.5f;
  s->geom = geom;
  s->compiled = split_compiled(R, K) &&
                fmd::split_geom(R, K, T, fmd::kSplitThreads, real).total * sizeof(float2) <= fmd::kSplitLdsBytes;
  s->taps = fmd::make_lanczos(K, cutoff);
  s->shifts.assign(shifts, shifts + size_t(n_captures) * n_bands);
  const size_t rows = size_t(n_captures) * n_bands;
  // (zero-filled: no sample in front of q = 0)
  const size_t nh = size_t(n_captures) * K;
  if (s->d_coeff.alloc(s->taps.size()) || s->d_luts.alloc(rows * T) ||
      (real ? s->d_rhist[0].alloc(nh) || s->d_rhist[1].alloc(nh) : s->d_hist[0].alloc(nh) || s->d_hist[1].alloc(nh)))
    return fail(FMD_ERR_DEVICE, f + ": device allocation failed");
  HIPCHK(hipMemcpy(s->d_coeff.p, s->taps.data(), s->taps.size() * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipDeviceSynchronize());
  *out = s.release();
  return FMD_OK;
}

} // namespace

extern "C" {

int fmd_split_create(const fmd_split_params* p, unsigned n_captures, unsigned n_bands, const int* shifts, int device,
                     fmd_split** out)
{
  return split_create("fmd_split_create", false, p, n_captures, n_bands, shifts, device, out);
}

int fmd_split_create_real(const fmd_split_params* p, unsigned n_captures, unsigned n_bands, const int* shifts,
                          int device, fmd_split** out)
{
  return split_create("fmd_split_create_real", true, p, n_captures, n_bands, shifts, device, out);
}

void fmd_split_destroy(fmd_split* s)
{
  if (s)
  {
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
  }
  delete s;
}

int fmd_split_reset(fmd_split* s, void* stream)
{
  if (!s)
    return fail(FMD_ERR_ARG, "fmd_split_reset: null splitter");
  HIPCHK(hipSetDevice(s->device));
  // (the buffer the next call reads; the other one is written whole before it is read)
  if (s->real)
    HIPCHK(hipMemsetAsync(s->d_rhist[s->parity].p, 0, size_t(s->G) * s->geom.K * sizeof(float),
                          static_cast<hipStream_t>(stream)));
  else
    HIPCHK(hipMemsetAsync(s->d_hist[s->parity].p, 0, size_t(s->G) * s->geom.K * sizeof(float2),
                          static_cast<hipStream_t>(stream)));
  s->q = 0;
  return FMD_OK;
}

int fmd_split_set_shifts(fmd_split* s, const int* shifts, unsigned n_rows)
{
  if (!s || !shifts)
    return fail(FMD_ERR_ARG, "fmd_split_set_shifts: null splitter or shifts");
  if (n_rows != s->G * s->B)
    return fail(FMD_ERR_ARG, "fmd_split_set_shifts: n_rows must be n_captures * n_bands");
  s->shifts.assign(shifts, shifts + n_rows);
  s->shifts_dirty = true; // the next call uploads the tables on its stream, in front of its kernel
  return FMD_OK;
}

int fmd_split_rows(const fmd_split* s)
{
  if (!s)
    return fail(FMD_ERR_ARG, "fmd_split_rows: null splitter");
  return int(s->G * s->B);
}

double fmd_split_out_rate(const fmd_split* s)
{
  if (!s)
  {
    fail(FMD_ERR_ARG, "fmd_split_out_rate: null splitter");
    return 0.0;
  }
  return s->fs / double(s->geom.R);
}

unsigned fmd_split_max_out_samples(const fmd_split* s, unsigned samples)
{
  if (!s)
  {
    fail(FMD_ERR_ARG, "fmd_split_max_out_samples: null splitter");
    return 0;
  }
  return unsigned((size_t(samples) + s->geom.R - 1) / s->geom.R);
}

int fmd_split_get_taps(const fmd_split* s, float* out, unsigned cap)
{
  if (!s || (!out && cap))
    return fail(FMD_ERR_ARG, "fmd_split_get_taps: null splitter or buffer");
  const unsigned K = s->geom.K;
  for (unsigned j = 0; j < K && j < cap; j++)
    out[j] = s->taps[j + 1];
  return int(K);
}

unsigned fmd_split_tile_samples(const fmd_split* s)
{
  if (!s)
  {
    fail(FMD_ERR_ARG, "fmd_split_tile_samples: null splitter");
    return 0;
  }
  return (s->compiled ? unsigned(fmd::kSplitThreads) : s->geom.TO) * s->geom.R;
}

int fmd_split_debug_table_versions(const fmd_split* s)
{
  if (!s)
    return fail(FMD_ERR_ARG, "fmd_split_debug_table_versions: null splitter");
  return int(s->pool.size());
}

int fmd_split_process_device(fmd_split* s, const void* d_in, int iq_format, size_t in_capture_stride, unsigned samples,
                             void* d_out, size_t out_row_stride, unsigned* out_samples, void* stream)
{
  if (int rc = split_check("fmd_split_process_device", s, d_in, iq_format, in_capture_stride, samples, d_out,
                           out_row_stride, true))
    return rc;
  return split_process(s, d_in, iq_format, in_capture_stride, samples, static_cast<float2*>(d_out),
                       out_row_stride, out_samples, static_cast<hipStream_t>(stream));
}

int fmd_split_process_host(fmd_split* s, const void* in, int iq_format, size_t in_capture_stride, unsigned samples,
                           void* out, size_t out_row_stride, unsigned* out_samples)
{
  if (int rc = split_check("fmd_split_process_host", s, in, iq_format, in_capture_stride, samples, out,
                           out_row_stride, false))
    return rc;
  HIPCHK(hipSetDevice(s->device));
  const size_t esz = s->real ? real_format_esz(iq_format) : format_esz(FMT_IQ, iq_format);
  const size_t rows = size_t(s->G) * s->B;
  // device rows: captures one behind the other at an even stride (real samples: a multiple of four), rows at the
  // even stride the kernel needs
  const size_t d_in_stride = s->real ? (size_t(samples) + 3) & ~size_t(3) : (size_t(samples) + 1) & ~size_t(1);
  const size_t d_out_stride = (size_t(fmd_split_max_out_samples(s, samples)) + 1) & ~size_t(1);
  const size_t in_bytes = s->G * d_in_stride * esz, out_bytes = rows * d_out_stride * sizeof(float2);
  if (in_bytes > s->d_stage_in.n || out_bytes > s->d_stage_out.n)
  {
    HIPCHK(hipStreamSynchronize(nullptr)); // the old buffers may still be in use by work queued on this stream
    if ((in_bytes > s->d_stage_in.n && s->d_stage_in.alloc(in_bytes)) ||
        (out_bytes > s->d_stage_out.n && s->d_stage_out.alloc(out_bytes)))
      return fail(FMD_ERR_DEVICE, "fmd_split: device allocation failed");
  }
  HIPCHK(hipMemcpy2D(s->d_stage_in.p, d_in_stride * esz, in, (s->G > 1 ? in_capture_stride : samples) * esz,
                     size_t(samples) * esz, s->G, hipMemcpyHostToDevice));
  unsigned M = 0;
  if (int rc = split_process(s, s->d_stage_in.p, iq_format, d_in_stride, samples,
                             reinterpret_cast<float2*>(s->d_stage_out.p), d_out_stride, &M, nullptr))
    return rc;
  HIPCHK(hipStreamSynchronize(nullptr));
  if (M)
    HIPCHK(hipMemcpy2D(out, (rows > 1 ? out_row_stride : M) * sizeof(float2), s->d_stage_out.p,
                       d_out_stride * sizeof(float2), size_t(M) * sizeof(float2), rows, hipMemcpyDeviceToHost));
  if (out_samples)
    *out_samples = M;
  return FMD_OK;
}

} // extern "C"
