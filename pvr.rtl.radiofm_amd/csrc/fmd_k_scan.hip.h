/*
 * fmd_k_scan.hip.h -- the band scan's kernels (fmd_scan_*, include/fmd.h): an averaged power spectrum of every
 * capture of a batch (k_scan_psd, k_scan_reduce) and its reading on the tuner raster (k_scan_slots).
 *
 * k_scan_psd: Welch segments of N samples at a hop of N/2, periodic Hann window, one N-point complex FFT per
 * segment.  The FFT is a Stockham autosort in radix-16 passes held in registers -- 16 elements per thread, N/16
 * threads per segment -- with the last pass of radix N/256 (N = 256: none):
 *     256 = 16 x 16, 512 = 16 x 16 x 2, 1024 = 16 x 16 x 4, 2048 = 16 x 16 x 8, 4096 = 16 x 16 x 16,
 * so a segment costs one LDS exchange (N = 256) or two.  The first pass reads the capture from HBM and windows it
 * as it arrives (each thread keeps its 16 window values in registers); the last pass adds |X|^2 into registers,
 * and a thread's bins are the same for every segment.  The half a segment shares with its neighbour is read a
 * second time, meant to come from L1 / L2 (not measured): the segments of a chunk run on the P = 256 / (N/16) subgroups side by
 * side, and one after another where P = 1.  Twiddles come from a float table the host computed in double.
 *
 * Summation tree (a function of N and the call's size alone):
 *   - a chunk is 16 consecutive segments of a call (the last chunk of a call may hold fewer); subgroup q takes
 *     segments q, q + P, ... of it and adds their |X|^2 in that order (float);
 *   - the chunk's partial = the P subgroup sums added in the order q = 0 .. P-1 (float);
 *   - the capture's running total (double, on the device) += partial, chunk by chunk, call by call.
 * Many captures: one workgroup per capture walks its chunks (no scratch).  Few captures: one workgroup per
 * (capture, chunk) writes the partial to a scratch buffer and k_scan_reduce adds them in chunk order -- the same
 * additions in the same order, so both forms give the same bits.
 */
#pragma once

#include "fmd_k_common.hip.h"
#include "fmd_k_if.hip.h" // InF32 / InU8 / InS8 / InS16: the decoder's input formats (fmd_u8_to_f32, fmd_s8_to_f32, ...)

namespace fmd
{

constexpr int kScanThreads = 256;
constexpr int kScanElems = 16;   // complex elements per thread and pass
constexpr int kScanChunk = 16;   // segments per chunk
constexpr int kScanMaxN = 4096;
constexpr int kScanMaxSlots = 1024;

/* LDS index with one pad element per 16: the radix-16 passes write 16 apart in the first pass */
__device__ __forceinline__ int scan_pad(int i) { return i + (i >> 4); }

__device__ __forceinline__ float2 scan_cmul(float2 a, float2 b)
{
  return make_float2(__builtin_fmaf(a.x, b.x, -(a.y * b.y)), __builtin_fmaf(a.x, b.y, a.y * b.x));
}

template <int R>
constexpr int scan_bitrev(int r)
{
  int o = 0;
  for (int m = 1; m < R; m <<= 1)
    o = (o << 1) | ((r & m) ? 1 : 0);
  return o;
}

/* In-register R-point DFT: v[q] <- sum_r v[r] exp(-2 pi i r q / R).  Radix-2 decimation in time; W_len^m is
 * tw[m N / len] of the N-point table (a compile-time index: one scalar load), W = 1 and W = -i exactly. */
template <int R, int N>
__device__ __forceinline__ void scan_dft(float2 (&v)[R], const float2* __restrict__ tw)
{
  float2 a[R];
#pragma unroll
  for (int r = 0; r < R; ++r)
    a[scan_bitrev<R>(r)] = v[r];
#pragma unroll
  for (int len = 2; len <= R; len *= 2)
#pragma unroll
    for (int s = 0; s < R; s += len)
#pragma unroll
      for (int m = 0; m < len / 2; ++m)
      {
        const float2 u = a[s + m];
        float2 t = a[s + m + len / 2];
        if (4 * m == len)
          t = make_float2(t.y, -t.x);
        else if (m != 0)
          t = scan_cmul(t, tw[m * (N / len)]);
        a[s + m] = make_float2(u.x + t.x, u.y + t.y);
        a[s + m + len / 2] = make_float2(u.x - t.x, u.y - t.y);
      }
#pragma unroll
  for (int r = 0; r < R; ++r)
    v[r] = a[r];
}

/* One Stockham pass of radix R after NS points (NS = product of the radices before it) on a segment in LDS: thread
 * t takes the butterflies j = t + b N/16 (b < 16/R).  Not LAST: the result goes back to LDS (all reads of the
 * pass are complete before the first write).  LAST: |X|^2 is added to acc[b R + q], bin (j/NS) NS R + j%NS + q NS. */
template <int N, int R, int NS, bool LAST>
__device__ __forceinline__ void scan_pass(float2* buf, int t, const float2* __restrict__ tw, float (&acc)[kScanElems],
                                          bool valid)
{
  constexpr int NT = N / kScanElems, B = kScanElems / R;
  float2 v[B][R];
#pragma unroll
  for (int b = 0; b < B; ++b)
#pragma unroll
    for (int r = 0; r < R; ++r)
      v[b][r] = buf[scan_pad(t + b * NT + r * (N / R))];
  if (!LAST)
    __syncthreads();
#pragma unroll
  for (int b = 0; b < B; ++b)
  {
    const int j = t + b * NT, k = j & (NS - 1);
    /* twiddle W^(r k) of element r, W = tw[k N / (NS R)]: W, W^2, W^4, W^8 from the table, the other powers as
     * products of those (at most three roundings) -- few registers stay live across the segment loop */
    float2 wp[5];
#pragma unroll
    for (int l = 0; (1 << l) < R; ++l)
      wp[l] = tw[(k << l) * (N / (NS * R))];
#pragma unroll
    for (int r = 1; r < R; ++r)
    {
      float2 w = make_float2(1.0f, 0.0f);
      bool first = true;
#pragma unroll
      for (int l = 0; (1 << l) < R; ++l)
        if (r & (1 << l))
        {
          w = first ? wp[l] : scan_cmul(w, wp[l]);
          first = false;
        }
      v[b][r] = scan_cmul(v[b][r], w);
    }
    scan_dft<R, N>(v[b], tw);
    const int o = (j / NS) * NS * R + k;
#pragma unroll
    for (int q = 0; q < R; ++q)
    {
      if (LAST)
      {
        if (valid)
          acc[b * R + q] += __builtin_fmaf(v[b][q].x, v[b][q].x, v[b][q].y * v[b][q].y);
      }
      else
        buf[scan_pad(o + q * NS)] = v[b][q];
    }
  }
}

/* FFT bin (natural order, 0 .. N-1) of acc[e] of thread t: the last pass's output index */
template <int N>
__device__ __forceinline__ int scan_bin(int t, int e)
{
  constexpr int NT = N / kScanElems;
  constexpr int R = (N == 256) ? 16 : N / 256, NS = N / R;
  const int b = e / R, q = e % R, j = t + b * NT, k = j & (NS - 1);
  return (j / NS) * NS * R + k + q * NS;
}

/* k_scan_psd: see the file comment.  Rows: capture g starts at iq + g * stride samples.  S segments in this call,
 * n_chunks = ceil(S / kScanChunk).  scratch == nullptr: grid = G, totals[g][bin] (double, natural FFT order) +=
 * every chunk in order.  Otherwise grid = (n_chunks, G): scratch[(g n_chunks + c) N + bin] = the chunk's partial. */
template <class In, int N>
__global__ __launch_bounds__(kScanThreads, 2) void k_scan_psd(const typename In::elem* __restrict__ iq, size_t stride,
                                                           unsigned S, unsigned n_chunks,
                                                           const float* __restrict__ win,
                                                           const float2* __restrict__ tw,
                                                           double* __restrict__ totals, float* __restrict__ scratch)
{
  constexpr int NT = N / kScanElems, P = kScanThreads / NT, hop = N / 2, PADN = N + N / 16;
  constexpr int BPT = N / kScanThreads; // bins per thread in the combine
  __shared__ float2 lds[P * PADN];
  const int tid = threadIdx.x, t = tid % NT, q = tid / NT;
  float2* buf = lds + q * PADN;
  float* part = reinterpret_cast<float*>(lds);

  const bool split = scratch != nullptr;
  const unsigned g = split ? blockIdx.y : blockIdx.x;
  const unsigned c0 = split ? blockIdx.x : 0u, c1 = split ? blockIdx.x + 1 : n_chunks;
  const typename In::elem* row = iq + size_t(g) * stride;

  float w[kScanElems];
#pragma unroll
  for (int r = 0; r < kScanElems; ++r)
    w[r] = win[t + r * NT];
  double dacc[BPT];
  if (!split)
#pragma unroll
    for (int m = 0; m < BPT; ++m)
      dacc[m] = totals[size_t(g) * N + tid + m * kScanThreads];

#pragma unroll 1
  for (unsigned c = c0; c < c1; ++c)
  {
    float acc[kScanElems];
#pragma unroll
    for (int e = 0; e < kScanElems; ++e)
      acc[e] = 0.0f;
#pragma unroll 1
    for (int it = 0; it < kScanChunk / P; ++it)
    {
      /* the twiddles are re-read every segment (L1 / scalar cache) instead of being hoisted out of the loop:
       * kept live they would cost ~100 registers and most of the occupancy */
      const float2* twl = tw;
      asm volatile("" : "+s"(twl));
      const unsigned s = c * kScanChunk + it * P + q;
      const bool valid = s < S;
      // pass 1 (radix 16 on samples t + r N/16, no twiddle): loads first, then wait for the LDS to be free
      float2 v[kScanElems];
      const typename In::elem* x = row + size_t(valid ? s : 0u) * hop;
#pragma unroll
      for (int r = 0; r < kScanElems; ++r)
      {
        const float2 a = valid ? In::one(x, t + r * NT) : make_float2(0.0f, 0.0f);
        v[r] = make_float2(a.x * w[r], a.y * w[r]);
      }
      scan_dft<16, N>(v, twl);
      __syncthreads();
#pragma unroll
      for (int r = 0; r < kScanElems; ++r)
        buf[scan_pad(t * 16 + r)] = v[r];
      __syncthreads();
      if constexpr (N == 256)
        scan_pass<N, 16, 16, true>(buf, t, twl, acc, valid);
      else
      {
        scan_pass<N, 16, 16, false>(buf, t, twl, acc, valid);
        __syncthreads();
        scan_pass<N, N / 256, 256, true>(buf, t, twl, acc, valid);
      }
    }
    // the chunk's partial: subgroup sums in the order q = 0 .. P-1
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kScanElems; ++e)
      part[q * N + scan_bin<N>(t, e)] = acc[e];
    __syncthreads();
#pragma unroll
    for (int m = 0; m < BPT; ++m)
    {
      const int bin = tid + m * kScanThreads;
      float sum = part[bin];
#pragma unroll
      for (int p = 1; p < P; ++p)
        sum += part[p * N + bin];
      if (split)
        scratch[(size_t(g) * n_chunks + c) * N + bin] = sum;
      else
        dacc[m] += double(sum);
    }
  }
  if (!split)
#pragma unroll
    for (int m = 0; m < BPT; ++m)
      totals[size_t(g) * N + tid + m * kScanThreads] = dacc[m];
}

/* The few-captures form's second half: totals[g][bin] += scratch chunk partials in chunk order. */
__global__ __launch_bounds__(256) void k_scan_reduce(double* __restrict__ totals, const float* __restrict__ scratch,
                                                     unsigned n_captures, unsigned N, unsigned n_chunks)
{
  const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= size_t(n_captures) * N)
    return;
  const size_t g = i / N, bin = i % N;
  double v = totals[i];
  for (unsigned c = 0; c < n_chunks; ++c)
    v += double(scratch[(g * n_chunks + c) * N + bin]);
  totals[i] = v;
}

/* One slot of the raster (host-computed, include/fmd.h fmd_scan_params): bins [blo, bhi] within half_width_hz of
 * its centre, eligible slots [nlo, nhi] within min_separation_hz (itself included). */
struct ScanSlot
{
  int blo, bhi, nlo, nhi;
  int eligible, shift;
  float offset_hz;
  int pad_;
};

struct ScanCandidate
{
  int32_t shift;
  float offset_hz, power_db, snr_db;
};

struct ScanSlotArgs
{
  const double* totals;
  const ScanSlot* slots;
  double denom;     // K N sum(w^2)
  unsigned N, T, floor_index, max_cand;
  float threshold_db;
  float* psd;       // [G][N] or null
  float* slot_db;   // [G][T] or null
  float* floor_db;  // [G] or null
  ScanCandidate* cand; // [G][max_cand] or null
  uint32_t* counts; // [G] or null
};

/* k_scan_slots: one workgroup per capture.  P (fft-shifted: bin i at (i - N/2) fs / N) = totals / denom rounded
 * to float; the floor bin by a bitonic sort in LDS; slot powers summed in double in bin order; the candidate rule of
 * include/fmd.h; candidates in order of increasing frequency (decreasing shift). */
__global__ __launch_bounds__(256) void k_scan_slots(ScanSlotArgs a)
{
  __shared__ float pu[kScanMaxN], ps[kScanMaxN];
  __shared__ double sp[kScanMaxSlots], snr[kScanMaxSlots];
  __shared__ unsigned char cand[kScanMaxSlots];
  const unsigned g = blockIdx.x, tid = threadIdx.x, N = a.N, T = a.T;
  const double* tot = a.totals + size_t(g) * N;
  for (unsigned i = tid; i < N; i += blockDim.x)
  {
    const float p = float(tot[(i + N / 2) & (N - 1)] / a.denom);
    pu[i] = p;
    ps[i] = p;
    if (a.psd)
      a.psd[size_t(g) * N + i] = p;
  }
  __syncthreads();
  for (unsigned k = 2; k <= N; k <<= 1)
    for (unsigned j = k >> 1; j > 0; j >>= 1)
    {
      for (unsigned i = tid; i < N; i += blockDim.x)
      {
        const unsigned l = i ^ j;
        if (l > i)
        {
          const float x = ps[i], y = ps[l];
          if ((x > y) == ((i & k) == 0))
          {
            ps[i] = y;
            ps[l] = x;
          }
        }
      }
      __syncthreads();
    }
  const double fb = double(ps[a.floor_index]);
  if (tid == 0 && a.floor_db)
    a.floor_db[g] = float(10.0 * log10(fb));
  for (unsigned j = tid; j < T; j += blockDim.x)
  {
    const ScanSlot s = a.slots[j];
    double p = 0.0, r = -INFINITY;
    if (s.eligible)
    {
      for (int i = s.blo; i <= s.bhi; ++i)
        p += double(pu[i]);
      r = 10.0 * log10(p / (fb * double(s.bhi - s.blo + 1)));
    }
    sp[j] = p;
    snr[j] = r;
    if (a.slot_db)
      a.slot_db[size_t(g) * T + j] = s.eligible ? float(10.0 * log10(p)) : -INFINITY;
  }
  __syncthreads();
  for (unsigned j = tid; j < T; j += blockDim.x)
  {
    const ScanSlot s = a.slots[j];
    bool ok = s.eligible && snr[j] >= double(a.threshold_db);
    for (int n = s.nlo; ok && n <= s.nhi; ++n)
      if (n != int(j) && a.slots[n].eligible)
        ok = (n < int(j)) ? sp[j] > sp[n] : sp[j] >= sp[n];
    cand[j] = ok;
  }
  __syncthreads();
  if (tid == 0)
  {
    unsigned n = 0;
    for (int j = int(T) - 1; j >= 0; --j)
    {
      if (!cand[j])
        continue;
      if (a.cand && n < a.max_cand)
      {
        const ScanSlot s = a.slots[j];
        ScanCandidate c;
        c.shift = s.shift;
        c.offset_hz = s.offset_hz;
        c.power_db = float(10.0 * log10(sp[j]));
        c.snr_db = float(snr[j]);
        a.cand[size_t(g) * a.max_cand + n] = c;
      }
      ++n;
    }
    if (a.counts)
      a.counts[g] = n;
  }
}

} // namespace fmd
