/*
 * fmd_chan.inc.hpp -- the polyphase channeliser's host side (fmd_chan_*, include/fmd.h): parameter checks, the taps,
 * the twiddle tables in the layout the matrix cores read, and the launches of csrc/fmd_k_chan.hip.h on the caller's
 * stream.  Included by fmd_batch.hip (one translation unit: it shares g_err / fail / HIPCHK); the kernels are in
 * fmd_chan.hip's object.  A channeliser owns no stream and no state of any fmd_batch.
 */
#include "fmd_k_chan.hip.h"

struct fmd_chan
{
  int device = 0;
  unsigned G = 0, B = 0;
  unsigned N = 0, D = 0, K = 0;
  bool real = false;                // fmd_chan_create_real: FMD_REAL_* input, the real forms of the kernels, for life
  unsigned nmb = 0;                 // blocks of 32 rows of the table per capture
  unsigned lds = 0;                 // bytes of a workgroup
  double fs = 0.0;
  float scale = 1.0f;
  unsigned long long q = 0;         // input samples of every capture since create / reset (host, call order)
  unsigned parity = 0;              // which history buffer the next call reads
  std::vector<float> taps;          // c[0 .. K + 1]
  std::vector<int> shifts;          // [G B], as the next call will use them
  bool shifts_dirty = true;         // the device table is not that of `shifts`
  DevBuf<float> d_coeff;
  DevBuf<float2> d_hist[2];         // [G][K] raw (converted) history, by call parity (real: G K floats in it)
  DevBuf<float> d_atab;             // [G][nmb][steps()][64]: written by an upload on the calls' stream, behind its last
                                    // reader
  /* page-locked staging of one version of the table, as the splitter's: set_shifts never waits */
  struct Staging
  {
    HostBuf<float> h;
    Event done;
    bool used = false;
  };
  std::vector<std::unique_ptr<Staging>> pool;
  DevBuf<char> d_stage_in, d_stage_out; // fmd_chan_process_host

  /* MFMA steps of a row block: a complex one has a step per branch, a real one a step per two (chan_real_steps) */
  unsigned steps() const { return real ? fmd::chan_real_steps(N).s0 + fmd::chan_real_steps(N).s1 : N; }
  size_t table_floats() const { return size_t(G) * nmb * steps() * 64; }
  size_t hist_bytes() const { return size_t(G) * K * (real ? sizeof(float) : sizeof(float2)); }
  ~fmd_chan() { (void)hipSetDevice(device); } // (the buffers free themselves behind it)
};

namespace
{

const char kChanFormats[] = "iq_format must be one of FMD_IQ_F32, _U8, _S8, _S16 (0..3)";
const char kChanRealFormats[] = "iq_format must be one of FMD_REAL_F32, _S8, _S16 (16, 18, 19)";
const char kChanOutFormats[] = "out_format must be FMD_CIQ_F32 or FMD_CIQ_S16 (0..1)";

/* outputs of a call of n samples behind q samples: the multiples of D in [q, q + n) */
inline unsigned chan_count(unsigned long long q, unsigned n, unsigned D, unsigned* pos)
{
  const unsigned p = unsigned((D - q % D) % D);
  if (pos)
    *pos = p;
  return n > p ? (n - p - 1) / D + 1 : 0u;
}

/* the argument checks of a process call that need no device */
int chan_check(const char* fn, fmd_chan* c, const void* in, int format, size_t in_stride, unsigned samples,
               const void* out, int out_format, size_t out_stride, bool device_call)
{
  const std::string f(fn);
  const bool real = c && c->real;
  if (real_format_ok(format))
  {
    if (!c)
      return fail(FMD_ERR_ARG, f + ": a channeliser takes no real-sampled input (FMD_REAL_*), " + kChanFormats);
    if (!real)
      return fail(FMD_ERR_ARG, f + ": this channeliser is a complex one (fmd_chan_create): it takes no real-sampled "
                                   "input (FMD_REAL_*), " + kChanFormats);
  }
  else if (format == FMD_IN_CIQ_F32 || format == FMD_IN_CIQ_S16)
    return fail(FMD_ERR_ARG, f + ": channel IQ rows (FMD_IN_CIQ_*) are what a channeliser makes, not its input, " +
                                 (real ? kChanRealFormats : kChanFormats));
  else if (!format_ok(FMT_IQ, format))
    return fail(FMD_ERR_ARG, f + ": " + (real ? kChanRealFormats : kChanFormats));
  else if (real)
    return fail(FMD_ERR_ARG, f + ": this channeliser is a real one (fmd_chan_create_real): it takes no complex input "
                                 "(FMD_IQ_*), " + kChanRealFormats);
  if (!format_ok(FMT_CIQ, out_format))
    return fail(FMD_ERR_ARG, f + ": " + kChanOutFormats);
  if (!c || !in || !out)
    return fail(FMD_ERR_ARG, f + ": null channeliser, input or output pointer");
  const bool s16 = out_format == FMD_CIQ_S16;
  if (samples == 0 || samples > FMD_CHAN_MAX_SAMPLES)
    return fail(FMD_ERR_SIZE, f + ": samples must be 1 .. FMD_CHAN_MAX_SAMPLES (16777216)");
  if (c->G > 1 && in_stride < samples)
    return fail(FMD_ERR_ARG, f + ": in_capture_stride is shorter than a capture (samples)");
  const unsigned M = chan_count(c->q, samples, c->D, nullptr);
  if (c->G * c->B > 1 && out_stride < M)
    return fail(FMD_ERR_ARG, f + ": out_row_stride is shorter than the call's output count");
  if (device_call)
  {
    if (real)
    {
      if (reinterpret_cast<uintptr_t>(in) % (4 * real_format_esz(format)) || (c->G > 1 && in_stride % 4))
        return fail(FMD_ERR_ARG, f + ": d_in and in_capture_stride must be multiples of four real samples");
    }
    else
    {
      const size_t pair = 2 * format_esz(FMT_IQ, format);
      if (reinterpret_cast<uintptr_t>(in) % pair || (c->G > 1 && in_stride % 2))
        return fail(FMD_ERR_ARG, f + ": d_in and in_capture_stride must be multiples of two IQ samples");
    }
    if (s16 && (reinterpret_cast<uintptr_t>(out) % 16 || out_stride % 4))
      return fail(FMD_ERR_ARG, f + ": d_out must be 16-byte aligned and out_row_stride a multiple of 4 complex "
                                   "samples (FMD_CIQ_S16)");
    if (reinterpret_cast<uintptr_t>(out) % 16 || out_stride % 2)
      return fail(FMD_ERR_ARG, f + ": d_out must be 16-byte aligned and out_row_stride even");
    if (out_stride < M)
      return fail(FMD_ERR_ARG, f + ": out_row_stride is shorter than the call's output count");
  }
  return FMD_OK;
}

/* W[r] = exp(+2 pi i s r / N), r = 0 .. N - 1, as (re, im) floats: the angle reduced in integers, cos and sin in
 * double, rounded once */
std::vector<float> chan_twiddles(unsigned N, int shift)
{
  const unsigned long long s = (unsigned long long)(((long long)shift % (long long)N + (long long)N) % (long long)N);
  std::vector<float> w(2 * size_t(N));
  for (unsigned r = 0; r < N; r++)
  {
    const double ang = 6.283185307179586476925286766559 * double((s * r) % N) / double(N);
    w[2 * r] = float(std::cos(ang));
    w[2 * r + 1] = float(std::sin(ang));
  }
  return w;
}

/* The table of c->shifts into d_atab, on the calls' stream in front of the next kernel.  Row b of capture g fills
 * rows i = 2 (b mod 16) (real part) and i + 1 (imaginary part) of block b / 16; step r holds the two k of branch r:
 * [r][0][i] meets Re U, [r][1][i] meets Im U.
 * A real channeliser has no Im U: a step holds two BRANCHES, [s][0][i] and [s][1][i] = W[2 s], W[2 s + 1] of the half
 * [0, N / 2) for s < s0, of the half [N / 2, N) behind it; the k of an odd half's padded step stays +0. */
int chan_upload_table(fmd_chan* c, hipStream_t stream)
{
  const unsigned N = c->N;
  const size_t total = c->table_floats();
  fmd_chan::Staging* st = nullptr;
  for (auto& p : c->pool)
    if (!p->used || hipEventQuery(p->done) == hipSuccess)
    {
      st = p.get();
      break;
    }
  if (!st)
  {
    std::unique_ptr<fmd_chan::Staging> p(new fmd_chan::Staging);
    if (p->h.alloc(total) || p->done.create() != hipSuccess)
      return fail(FMD_ERR_DEVICE, "fmd_chan: page-locked allocation failed");
    st = p.get();
    c->pool.push_back(std::move(p));
  }
  std::memset(st->h.p, 0, total * sizeof(float)); // (the rows behind B of the last block stay zero)
  std::map<int, std::vector<float>> by_shift;
  for (unsigned g = 0; g < c->G; g++)
    for (unsigned b = 0; b < c->B; b++)
    {
      const int s = int(((long long)c->shifts[size_t(g) * c->B + b] % (long long)N + (long long)N) % (long long)N);
      auto it = by_shift.find(s);
      if (it == by_shift.end())
        it = by_shift.emplace(s, chan_twiddles(N, s)).first;
      const float* w = it->second.data();
      float* t = st->h.p + (size_t(g) * c->nmb + b / 16) * c->steps() * 64 + 2 * (b % 16);
      if (c->real)
      {
        const unsigned Nh = N / 2, s0 = fmd::chan_real_steps(N).s0;
        for (unsigned r = 0; r < N; r++)
        {
          const unsigned i = r < Nh ? r : r - Nh; // the branch's place in its half
          float* e = t + (size_t(r < Nh ? 0 : s0) + i / 2) * 64 + 32 * (i % 2);
          e[0] = w[2 * r];     // Re y += U * Wre
          e[1] = w[2 * r + 1]; // Im y += U * Wim
        }
        continue;
      }
      for (unsigned r = 0; r < N; r++, t += 64)
      {
        const float re = w[2 * r], im = w[2 * r + 1];
        t[0] = re;       // Re y += Re U * Wre
        t[32] = -im;     //       += Im U * -Wim
        t[1] = im;       // Im y += Re U * Wim
        t[33] = re;      //       += Im U * Wre
      }
    }
  HIPCHK(hipMemcpyAsync(c->d_atab.p, st->h.p, total * sizeof(float), hipMemcpyHostToDevice, stream));
  HIPCHK(hipEventRecord(st->done, stream));
  st->used = true;
  c->shifts_dirty = false;
  return FMD_OK;
}

int chan_process(fmd_chan* c, const void* d_in, int fmt, size_t in_stride, unsigned samples, void* d_out,
                 int out_fmt, size_t out_stride, unsigned* out_samples, hipStream_t stream)
{
  HIPCHK(hipSetDevice(c->device));
  if (c->shifts_dirty)
    if (int rc = chan_upload_table(c, stream))
      return rc;
  fmd::ChanArgs a{};
  a.in = d_in;
  a.in_stride = c->G > 1 ? in_stride : 0;
  a.hist = c->d_hist[c->parity].p;
  a.atab = c->d_atab.p;
  a.coeff = c->d_coeff.p;
  a.out = static_cast<float2*>(d_out);
  a.out_stride = out_stride;
  a.n_in = samples;
  a.B = c->B;
  a.M = chan_count(c->q, samples, c->D, &a.pos);
  a.q0_mod = unsigned(c->q % c->N);
  a.scale2 = 2.0f * c->scale;
  a.N = c->N;
  a.D = c->D;
  a.K = c->K;
  if (a.M)
    fmd::chan_launch(fmt, out_fmt == FMD_CIQ_S16, (a.M + fmd::kChanTile - 1) / fmd::kChanTile, c->G, c->lds, stream, a);
  fmd::chan_roll(fmt, c->G, c->K, d_in, a.in_stride, samples, c->d_hist[c->parity].p, c->d_hist[c->parity ^ 1u].p,
                 stream);
  HIPCHK(hipGetLastError());
  c->parity ^= 1u;
  c->q += samples;
  if (out_samples)
    *out_samples = a.M;
  return FMD_OK;
}

/* fmd_chan_create / fmd_chan_create_real */
int chan_create(const char* fn, bool real, const fmd_chan_params* p, unsigned n_captures, unsigned n_rows_per_capture,
                const int* shifts, int device, fmd_chan** out)
{
  const std::string f(fn);
  if (!p || !out || !shifts)
    return fail(FMD_ERR_ARG, f + ": null argument (params, shifts or out)");
  *out = nullptr;
  if (n_captures == 0 || n_captures > 65535u)
    return fail(FMD_ERR_ARG, f + ": n_captures must be 1 .. 65535");
  if (n_rows_per_capture == 0 || size_t(n_captures) * n_rows_per_capture > (size_t(1) << 20))
    return fail(FMD_ERR_ARG,
                f + ": n_rows_per_capture must be at least 1 and n_captures * n_rows_per_capture at most 2^20");
  const double fs = p->sample_rate_in;
  if (!(fs > 0.0) || !std::isfinite(fs))
    return fail(FMD_ERR_ARG, f + ": sample_rate_in must be a positive rate");
  const unsigned N = p->n_bins;
  if (N < 2 || N > (real ? 512u : 256u))
    return fail(FMD_ERR_ARG, f + (real ? ": n_bins must be 2 .. 512" : ": n_bins must be 2 .. 256"));
  const unsigned D = p->decimation;
  if (D < 2 || D > 256)
    return fail(FMD_ERR_ARG, f + ": decimation must be 2 .. 256");
  const unsigned K = p->filter_order ? p->filter_order : 8 * D;
  if (K < 2 || K > 4096)
    return fail(FMD_ERR_ARG, f + ": filter_order must be 2 .. 4096 (0 = 8 * decimation)");
  const double cutoff = p->cutoff != 0.0 ? p->cutoff : 0.6 / double(D);
  if (!(cutoff > 0.0 && cutoff <= 0.5))
    return fail(FMD_ERR_ARG, f + ": cutoff must lie in (0, 0.5] of the input rate (0 = 0.6 / decimation)");
  if (!std::isfinite(p->out_scale))
    return fail(FMD_ERR_ARG, f + ": out_scale must be a finite float (0 = 1.0)");
  const unsigned lds =
      (real ? fmd::chan_real_geom(N, D, K).total : fmd::chan_geom(N, D, K).total) * unsigned(sizeof(float));
  if (lds > fmd::kChanLdsBytes)
    return fail(FMD_ERR_ARG, f + ": n_bins, decimation and filter_order: the window of a tile (31 * decimation + "
                                 "filter_order samples) and its n_bins branch sums do not fit a workgroup's LDS");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(FMD_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= ndev)
    return fail(FMD_ERR_ARG, f + ": device ordinal out of range");
  if (!fmd::chan_prepare || !fmd::chan_launch || !fmd::chan_roll) // (never in the library: fmd_k_chan.hip.h)
    return fail(FMD_ERR_DEVICE, f + ": the channeliser's kernels (fmd_chan.o) are not linked into this program");
  HIPCHK(hipSetDevice(device));
  if (int e = fmd::chan_prepare(fmd::kChanLdsBytes))
    return fail(FMD_ERR_DEVICE, f + ": hipFuncSetAttribute: " + hipGetErrorString(hipError_t(e)));
  std::unique_ptr<fmd_chan> c(new fmd_chan);
  c->device = device;
  c->G = n_captures;
  c->B = n_rows_per_capture;
  c->N = N;
  c->D = D;
  c->K = K;
  c->real = real;
  c->nmb = fmd::chan_row_blocks(c->B);
  c->lds = lds;
  c->fs = fs;
  c->scale = p->out_scale != 0.0f ? p->out_scale : 1.0f;
  c->taps = fmd::make_lanczos(K, cutoff);
  c->shifts.assign(shifts, shifts + size_t(n_captures) * n_rows_per_capture);
  const size_t nh = (c->hist_bytes() + sizeof(float2) - 1) / sizeof(float2); // (zero-filled: no sample before q = 0)
  if (c->d_coeff.alloc(c->taps.size()) || c->d_atab.alloc(c->table_floats()) || c->d_hist[0].alloc(nh) ||
      c->d_hist[1].alloc(nh))
    return fail(FMD_ERR_DEVICE, f + ": device allocation failed");
  HIPCHK(hipMemcpy(c->d_coeff.p, c->taps.data(), c->taps.size() * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipDeviceSynchronize());
  *out = c.release();
  return FMD_OK;
}

} // namespace

extern "C" {

int fmd_chan_create(const fmd_chan_params* p, unsigned n_captures, unsigned n_rows_per_capture, const int* shifts,
                    int device, fmd_chan** out)
{
  return chan_create("fmd_chan_create", false, p, n_captures, n_rows_per_capture, shifts, device, out);
}

int fmd_chan_create_real(const fmd_chan_params* p, unsigned n_captures, unsigned n_rows_per_capture, const int* shifts,
                         int device, fmd_chan** out)
{
  return chan_create("fmd_chan_create_real", true, p, n_captures, n_rows_per_capture, shifts, device, out);
}

void fmd_chan_destroy(fmd_chan* c)
{
  if (c)
  {
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
  }
  delete c;
}

int fmd_chan_reset(fmd_chan* c, void* stream)
{
  if (!c)
    return fail(FMD_ERR_ARG, "fmd_chan_reset: null channeliser");
  HIPCHK(hipSetDevice(c->device));
  // (the buffer the next call reads; the other one is written whole before it is read)
  HIPCHK(hipMemsetAsync(c->d_hist[c->parity].p, 0, c->hist_bytes(),
                        static_cast<hipStream_t>(stream)));
  c->q = 0;
  return FMD_OK;
}

int fmd_chan_set_shifts(fmd_chan* c, const int* shifts, unsigned n_rows)
{
  if (!c || !shifts)
    return fail(FMD_ERR_ARG, "fmd_chan_set_shifts: null channeliser or shifts");
  if (n_rows != c->G * c->B)
    return fail(FMD_ERR_ARG, "fmd_chan_set_shifts: n_rows must be n_captures * n_rows_per_capture");
  c->shifts.assign(shifts, shifts + n_rows);
  c->shifts_dirty = true; // the next call uploads the table on its stream, in front of its kernel
  return FMD_OK;
}

int fmd_chan_rows(const fmd_chan* c)
{
  if (!c)
    return fail(FMD_ERR_ARG, "fmd_chan_rows: null channeliser");
  return int(c->G * c->B);
}

double fmd_chan_out_rate(const fmd_chan* c)
{
  if (!c)
  {
    fail(FMD_ERR_ARG, "fmd_chan_out_rate: null channeliser");
    return 0.0;
  }
  return c->fs / double(c->D);
}

unsigned fmd_chan_max_out_samples(const fmd_chan* c, unsigned samples)
{
  if (!c)
  {
    fail(FMD_ERR_ARG, "fmd_chan_max_out_samples: null channeliser");
    return 0;
  }
  return unsigned((size_t(samples) + c->D - 1) / c->D);
}

int fmd_chan_get_taps(const fmd_chan* c, float* out, unsigned cap)
{
  if (!c || (!out && cap))
    return fail(FMD_ERR_ARG, "fmd_chan_get_taps: null channeliser or buffer");
  for (unsigned j = 0; j < c->K && j < cap; j++)
    out[j] = c->taps[j + 1];
  return int(c->K);
}

unsigned fmd_chan_tile_samples(const fmd_chan* c)
{
  if (!c)
  {
    fail(FMD_ERR_ARG, "fmd_chan_tile_samples: null channeliser");
    return 0;
  }
  return fmd::kChanTile * c->D;
}

int fmd_chan_process_device_fmt(fmd_chan* c, const void* d_in, int iq_format, size_t in_capture_stride,
                                unsigned samples, void* d_out, int out_format, size_t out_row_stride,
                                unsigned* out_samples, void* stream)
{
  if (int rc = chan_check("fmd_chan_process_device_fmt", c, d_in, iq_format, in_capture_stride, samples, d_out,
                          out_format, out_row_stride, true))
    return rc;
  return chan_process(c, d_in, iq_format, in_capture_stride, samples, d_out, out_format, out_row_stride, out_samples,
                      static_cast<hipStream_t>(stream));
}

int fmd_chan_process_device(fmd_chan* c, const void* d_in, int iq_format, size_t in_capture_stride, unsigned samples,
                            void* d_out, size_t out_row_stride, unsigned* out_samples, void* stream)
{
  if (int rc = chan_check("fmd_chan_process_device", c, d_in, iq_format, in_capture_stride, samples, d_out,
                          FMD_CIQ_F32, out_row_stride, true))
    return rc;
  return chan_process(c, d_in, iq_format, in_capture_stride, samples, d_out, FMD_CIQ_F32, out_row_stride,
                      out_samples, static_cast<hipStream_t>(stream));
}

} // extern "C"

namespace
{

/* fmd_chan_process_host / _host_fmt behind their checks */
int chan_process_host(fmd_chan* c, const void* in, int iq_format, size_t in_capture_stride, unsigned samples,
                      void* out, int out_format, size_t out_row_stride, unsigned* out_samples)
{
  HIPCHK(hipSetDevice(c->device));
  const size_t esz = c->real ? real_format_esz(iq_format) : format_esz(FMT_IQ, iq_format);
  const size_t osz = format_esz(FMT_CIQ, out_format);
  const size_t rows = size_t(c->G) * c->B;
  // device rows: captures one behind the other at the stride the kernel's loads need (two IQ samples, four real ones),
  // rows at the stride its stores need (even; S16: a multiple of 4)
  const size_t in_al = c->real ? 3 : 1, out_al = out_format == FMD_CIQ_S16 ? 3 : 1;
  const size_t d_in_stride = (size_t(samples) + in_al) & ~in_al;
  const size_t d_out_stride = (size_t(fmd_chan_max_out_samples(c, samples)) + out_al) & ~out_al;
  const size_t in_bytes = c->G * d_in_stride * esz, out_bytes = rows * d_out_stride * osz;
  if (in_bytes > c->d_stage_in.n || out_bytes > c->d_stage_out.n)
  {
    HIPCHK(hipStreamSynchronize(nullptr)); // the old buffers may still be in use by work queued on this stream
    if ((in_bytes > c->d_stage_in.n && c->d_stage_in.alloc(in_bytes)) ||
        (out_bytes > c->d_stage_out.n && c->d_stage_out.alloc(out_bytes)))
      return fail(FMD_ERR_DEVICE, "fmd_chan: device allocation failed");
  }
  HIPCHK(hipMemcpy2D(c->d_stage_in.p, d_in_stride * esz, in, (c->G > 1 ? in_capture_stride : samples) * esz,
                     size_t(samples) * esz, c->G, hipMemcpyHostToDevice));
  unsigned M = 0;
  if (int rc = chan_process(c, c->d_stage_in.p, iq_format, d_in_stride, samples, c->d_stage_out.p, out_format,
                            d_out_stride, &M, nullptr))
    return rc;
  HIPCHK(hipStreamSynchronize(nullptr));
  if (M)
    HIPCHK(hipMemcpy2D(out, (rows > 1 ? out_row_stride : M) * osz, c->d_stage_out.p, d_out_stride * osz,
                       size_t(M) * osz, rows, hipMemcpyDeviceToHost));
  if (out_samples)
    *out_samples = M;
  return FMD_OK;
}

} // namespace

extern "C" {

int fmd_chan_process_host_fmt(fmd_chan* c, const void* in, int iq_format, size_t in_capture_stride, unsigned samples,
                              void* out, int out_format, size_t out_row_stride, unsigned* out_samples)
{
  if (int rc = chan_check("fmd_chan_process_host_fmt", c, in, iq_format, in_capture_stride, samples, out, out_format,
                          out_row_stride, false))
    return rc;
  return chan_process_host(c, in, iq_format, in_capture_stride, samples, out, out_format, out_row_stride, out_samples);
}

int fmd_chan_process_host(fmd_chan* c, const void* in, int iq_format, size_t in_capture_stride, unsigned samples,
                          void* out, size_t out_row_stride, unsigned* out_samples)
{
  if (int rc = chan_check("fmd_chan_process_host", c, in, iq_format, in_capture_stride, samples, out, FMD_CIQ_F32,
                          out_row_stride, false))
    return rc;
  return chan_process_host(c, in, iq_format, in_capture_stride, samples, out, FMD_CIQ_F32, out_row_stride,
                           out_samples);
}

} // extern "C"
