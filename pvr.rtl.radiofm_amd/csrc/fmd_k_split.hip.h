/*
 * fmd_k_split.hip.h -- the band splitter's kernels (fmd_split_*, include/fmd.h): every wideband capture mixed and
 * decimated once into B bands at fs / R, each band the reference's cFineTuner + cDownsampleFilter::Process(complex)
 * (FmDecode.cpp:45-82, DownConvert.cpp:98-154) at a small integer decimation.  DESIGN.md section 9.13.
 *
 * k_split: one workgroup = one capture x one tile of TO <= 256 consecutive outputs, for ALL B bands of the capture.
 *   1. The tile's raw window -- (TO - 1) R + K input samples, the carried history in front of a call's first ones --
 *      is converted (InF32 / InU8 / InS8 / InS16, two samples per load where both lie in the call) and staged in LDS
 *      once.
 *   2. Per band: every window sample is multiplied with the band's tuner table ONCE into a second LDS window (never
 *      per tap); the table index steps and wraps (no division per sample: one remainder per lane and tile), the
 *      table of the band lives in LDS, the next band's is fetched while this band is mixed.
 *   3. One lane per output: the sum over taps j = 1 .. K in the reference's order, a rounded multiply and a rounded
 *      add per tap and part (packed: real and imaginary part in one v_pk_mul_f32 / v_pk_add_f32; the library is
 *      built with -ffp-contract=off), taps by scalar loads, then * out_scale and one 8-byte store.
 *   The mixed window is stored de-interleaved like the IF stage's (fmd_k_if.hip.h): slot i lives in region i mod 2^E
 *   at position i >> E, 2^E the power-of-two factor of R, so the lanes of a wave -- R samples apart -- read one region
 *   at an odd stride: conflict-free ds_read_b64.
 * k_split_roll: the raw history of the next call, the last K samples of (old history ++ this call's input), into the
 *   other of two history buffers: no reader of the old history is disturbed, and stream order puts it in front of
 *   the next call.
 * Nothing here depends on the grid: a row's bits are those of the definition whatever the tiling.
 *
 * k_split_real / k_split_roll_real: the same for real-sampled captures (FMD_REAL_*, fmd_split_create_real; DESIGN.md
 *   section 9.14), x[q] = (v[q], +0).  The raw window and the carried history hold one float a sample (InRealF32 /
 *   InRealS8 / InRealS16: four samples per load where all four lie in the call), so the generic form's tile is larger
 *   than the complex form's; the mix is t = (v lut.re, v lut.im), ONE packed multiply -- the two products with the zero
 *   part and the two sums that only add them are never formed.  They could change a bit only where v lut.re or
 *   v lut.im is a zero (its sign then depends on the zero product), and a zero of either sign times a tap is a zero
 *   added to a sum that starts at +0.0f and so is never -0: the sum does not see it.  Mixed window, tap loop, scale
 *   and store are k_split's (split_taps).
 */
#pragma once

namespace fmd
{

constexpr int kSplitThreads = 256;
constexpr unsigned kSplitLdsBytes = 65536;

/* Where a tile's LDS windows lie (float2 units), from (R, K, T, TO) alone -- the host and the compile-time forms of
 * the kernel compute the same. */
struct SplitGeom
{
  unsigned R, K, T, TO; // decimation, order, table size, outputs per tile (<= kSplitThreads)
  unsigned E;           // log2 of the power-of-two factor of R
  unsigned RS;          // float2 per region of the mixed window (odd: the regions start on different banks)
  unsigned off_mixed;   // raw window: [0, W), W = (TO - 1) R + K
  unsigned off_lut;     // two tables of T entries
  unsigned total;       // float2 in all
};
__host__ __device__ constexpr SplitGeom split_geom(unsigned R, unsigned K, unsigned T, unsigned TO, bool real = false)
{
  SplitGeom g{};
  g.R = R;
  g.K = K;
  g.T = T;
  g.TO = TO;
  unsigned e = 0;
  while (!((R >> e) & 1u))
    e++;
  g.E = e;
  const unsigned W = (TO - 1) * R + K;
  g.RS = ((W + (1u << e) - 1) >> e) | 1u;
  g.off_mixed = real ? (((W + 1u) >> 1) + 1u) & ~1u : (W + 1u) & ~1u; // (a real window: one float a sample)
  g.off_lut = (g.off_mixed + (g.RS << e) + 1u) & ~1u;
  g.total = g.off_lut + 2 * T;
  return g;
}

struct SplitArgs
{
  const void* in;         // capture g at in + g * in_stride elements
  size_t in_stride;
  const void* hist;       // [G][K] float2 (float: the real forms): x[q0 - K .. q0) of every capture, converted
  const float2* luts;     // [G B][T]
  const float* coeff;     // c[0 .. K + 1], taps c[1 .. K]
  float2* out;            // row r at out + r * out_stride
  size_t out_stride;
  unsigned N;             // input samples of the call
  unsigned B;             // bands per capture
  unsigned pos;           // the call's first output sits on input sample pos (q0 + pos is a multiple of R)
  unsigned M;             // outputs of the call
  unsigned lut_k;         // (q0 - K) mod T: the table index of the window sample K in front of the call
  unsigned lut_step;      // kSplitThreads mod T
  float scale;
  SplitGeom g;
};

/* RT, KT != 0: the geometry at compile time (TO = kSplitThreads, any T): the tap loop unrolls into immediate LDS
 * offsets.  RT = KT = 0: everything from a.g. */
template <class IN, int RT, int KT>
__global__ __launch_bounds__(kSplitThreads) void k_split(const SplitArgs a)
{
  typedef typename IN::pair pair_t;
  typedef typename IN::elem elem_t;
  constexpr int NT = kSplitThreads;
  constexpr bool CT = RT != 0;
  constexpr SplitGeom cg = split_geom(CT ? RT : 2, CT ? KT : 2, 1, NT);
  const unsigned R = CT ? cg.R : a.g.R, K = CT ? cg.K : a.g.K, TO = CT ? cg.TO : a.g.TO;
  const unsigned E = CT ? cg.E : a.g.E, RS = CT ? cg.RS : a.g.RS, off_mixed = CT ? cg.off_mixed : a.g.off_mixed;
  const unsigned off_lut = CT ? cg.off_lut : a.g.off_lut; // (T only moves the total)
  const unsigned T = a.g.T, emask = (1u << E) - 1u;
  extern __shared__ __attribute__((aligned(16))) float2 split_lds[];
  float2* const raw = split_lds;
  float2* const mixed = split_lds + off_mixed;
  float2* const lutS = split_lds + off_lut;

  const unsigned tid = threadIdx.x, g = blockIdx.y;
  const unsigned m0 = blockIdx.x * TO;
  const unsigned nout = min(TO, a.M - m0);
  const int p_first = (int)(a.pos + m0 * R);      // input sample of the tile's first output
  const int k_lo = p_first - (int)K;              // the window: samples k_lo .. k_hi of the call (k < 0: history)
  const int k_hi = p_first + (int)((nout - 1) * R) - 1;
  const unsigned Wt = (unsigned)(k_hi - k_lo + 1);
  const elem_t* __restrict__ x = static_cast<const elem_t*>(a.in) + uniform_u64((size_t)g * a.in_stride);
  const float2* __restrict__ h = static_cast<const float2*>(a.hist) + (size_t)g * K;

  // 1. the raw window, once for all bands
  {
    const int k_al = k_lo & ~1;
    const int npairs = (k_hi - k_al + 2) >> 1;
    const pair_t* __restrict__ xp = reinterpret_cast<const pair_t*>(x);
    for (int u = (int)tid; u < npairs; u += NT)
    {
      const int ka = k_al + 2 * u;
      if (ka >= 0 && ka + 1 < (int)a.N)
      {
        float2 s0, s1;
        IN::unpack(xp[ka >> 1], s0, s1);
        if (ka >= k_lo)
          raw[ka - k_lo] = s0;
        if (ka + 1 <= k_hi)
          raw[ka + 1 - k_lo] = s1;
      }
      else
      {
        for (int kk = ka; kk <= ka + 1; kk++)
          if (kk >= k_lo && kk <= k_hi) // (k_hi < N: an output needs nothing behind the sample in front of it)
            raw[kk - k_lo] = kk < 0 ? h[(int)K + kk] : IN::one(x, (size_t)kk);
      }
    }
  }
  const float2* __restrict__ lg = a.luts + (size_t)g * a.B * T;
  for (unsigned i = tid; i < T; i += NT)
    lutS[i] = lg[i];
  // the table index of window slot tid: one remainder per lane and tile, stepped and wrapped from there on
  const unsigned idx0 = (a.lut_k + (unsigned)p_first + tid) % T;
  const float* __restrict__ coeff = a.coeff;
  const fmd_f2v scale2 = {a.scale, a.scale};
  __syncthreads();

  for (unsigned b = 0; b < a.B; b++)
  {
    // 2. mix every window sample once; fetch the next band's table
    const float2* ls = lutS + (b & 1u) * T;
    unsigned idx = idx0;
    for (unsigned i = tid; i < Wt; i += NT)
    {
      mixed[(i & emask) * RS + (i >> E)] = cmul_pk(raw[i], ls[idx]);
      idx += a.lut_step;
      if (idx >= T)
        idx -= T;
    }
    if (b + 1 < a.B)
    {
      float2* ln = lutS + ((b + 1u) & 1u) * T;
      for (unsigned i = tid; i < T; i += NT)
        ln[i] = lg[(size_t)(b + 1) * T + i];
    }
    __syncthreads();
    // 3. one lane per output: taps j = 1 .. K in order; tap j reads window slot o R + K - j
    if (tid < nout)
    {
      fmd_f2v acc = {0.0f, 0.0f};
      const float2* w = mixed + tid * (R >> E);
      if constexpr (CT)
      {
#pragma unroll
        for (unsigned j = 1; j <= K; j++)
        {
          const unsigned c = K - j;
          const float2 sm = w[(c & emask) * RS + (c >> E)];
          const float cj = coeff[j];
          acc = acc + fmd_f2v{sm.x, sm.y} * fmd_f2v{cj, cj};
        }
      }
      else
      {
#pragma unroll 4
        for (unsigned j = 1; j <= K; j++)
        {
          const unsigned c = K - j;
          const float2 sm = w[(c & emask) * RS + (c >> E)];
          const float cj = coeff[j];
          acc = acc + fmd_f2v{sm.x, sm.y} * fmd_f2v{cj, cj};
        }
      }
      acc = acc * scale2;
      a.out[((size_t)g * a.B + b) * a.out_stride + m0 + tid] = make_float2(acc.x, acc.y);
    }
    __syncthreads(); // this band's window reads are done before the next band is mixed over them
  }
}

/* The next call's raw history: ho[i] = x[q0 + N - K + i], from the old history where the call was shorter than K. */
template <class IN>
__global__ __launch_bounds__(256) void k_split_roll(const void* in, size_t in_stride, unsigned N,
                                                    const float2* __restrict__ hist_in,
                                                    float2* __restrict__ hist_out, unsigned K)
{
  typedef typename IN::elem elem_t;
  const unsigned g = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
  if (i >= K)
    return;
  const elem_t* __restrict__ x = static_cast<const elem_t*>(in) + (size_t)g * in_stride;
  const unsigned keep = N < K ? K - N : 0u;
  hist_out[(size_t)g * K + i] = i < keep ? hist_in[(size_t)g * K + i + N] : IN::one(x, (size_t)(N + i - K));
}

/* Real-sampled input (FMD_REAL_*): one element per sample, converted like the I part of the matching FMD_IQ_*.  A
 * lane loads four samples at a time -- 16 bytes of float, 4 of signed bytes, 8 of signed 16-bit -- where all four lie
 * in the call (the call's pointer and capture stride are multiples of four samples), single samples at the window's
 * edges. */
struct InRealF32
{
  typedef float elem;
  typedef uint4 quad;
  static __device__ __forceinline__ float one(const elem* x, size_t k) { return x[k]; }
  static __device__ __forceinline__ void unpack(const quad& v, float (&s)[4])
  {
    s[0] = __uint_as_float(v.x);
    s[1] = __uint_as_float(v.y);
    s[2] = __uint_as_float(v.z);
    s[3] = __uint_as_float(v.w);
  }
};
struct InRealS8
{
  typedef signed char elem;
  typedef unsigned quad;
  static __device__ __forceinline__ float one(const elem* x, size_t k) { return fmd_s8_to_f32(x[k]); }
  static __device__ __forceinline__ void unpack(const quad& v, float (&s)[4])
  { // shift the byte to the top, then an arithmetic shift back: sign extension
    s[0] = fmd_s8_to_f32((int)(v << 24) >> 24);
    s[1] = fmd_s8_to_f32((int)(v << 16) >> 24);
    s[2] = fmd_s8_to_f32((int)(v << 8) >> 24);
    s[3] = fmd_s8_to_f32((int)v >> 24);
  }
};
struct InRealS16
{
  typedef short elem;
  typedef uint2 quad;
  static __device__ __forceinline__ float one(const elem* x, size_t k) { return fmd_s16_to_f32(x[k]); }
  static __device__ __forceinline__ void unpack(const quad& v, float (&s)[4])
  {
    s[0] = fmd_s16_to_f32((int)(v.x << 16) >> 16);
    s[1] = fmd_s16_to_f32((int)v.x >> 16);
    s[2] = fmd_s16_to_f32((int)(v.y << 16) >> 16);
    s[3] = fmd_s16_to_f32((int)v.y >> 16);
  }
};

/* One output of a real form: k_split's step 3 -- the sum over taps j = 1 .. K in order, tap j reads window slot
 * o R + K - j (w: the lane's slot 0 of the de-interleaved mixed window), then * out_scale and the 8-byte store.  CT:
 * K = KT at compile time.  (k_split keeps the text in its body: moved in here it compiled to other instructions.) */
template <bool CT, int KT>
__device__ __forceinline__ void split_taps(const float2* w, const float* __restrict__ coeff, unsigned K_,
                                           unsigned emask, unsigned RS, unsigned E, fmd_f2v scale2, float2* o)
{
  const unsigned K = CT ? (unsigned)KT : K_;
  fmd_f2v acc = {0.0f, 0.0f};
  if constexpr (CT)
  {
#pragma unroll
    for (unsigned j = 1; j <= K; j++)
    {
      const unsigned c = K - j;
      const float2 sm = w[(c & emask) * RS + (c >> E)];
      const float cj = coeff[j];
      acc = acc + fmd_f2v{sm.x, sm.y} * fmd_f2v{cj, cj};
    }
  }
  else
  {
#pragma unroll 4
    for (unsigned j = 1; j <= K; j++)
    {
      const unsigned c = K - j;
      const float2 sm = w[(c & emask) * RS + (c >> E)];
      const float cj = coeff[j];
      acc = acc + fmd_f2v{sm.x, sm.y} * fmd_f2v{cj, cj};
    }
  }
  acc = acc * scale2;
  *o = make_float2(acc.x, acc.y);
}

/* k_split for a real capture: a.g is split_geom(.., real = true), a.hist float [G][K], a.in / a.in_stride / a.N in
 * real samples. */
template <class IN, int RT, int KT>
__global__ __launch_bounds__(kSplitThreads) void k_split_real(const SplitArgs a)
{
  typedef typename IN::quad quad_t;
  typedef typename IN::elem elem_t;
  constexpr int NT = kSplitThreads;
  constexpr bool CT = RT != 0;
  constexpr SplitGeom cg = split_geom(CT ? RT : 2, CT ? KT : 2, 1, NT, true);
  const unsigned R = CT ? cg.R : a.g.R, K = CT ? cg.K : a.g.K, TO = CT ? cg.TO : a.g.TO;
  const unsigned E = CT ? cg.E : a.g.E, RS = CT ? cg.RS : a.g.RS, off_mixed = CT ? cg.off_mixed : a.g.off_mixed;
  const unsigned off_lut = CT ? cg.off_lut : a.g.off_lut;
  const unsigned T = a.g.T, emask = (1u << E) - 1u;
  extern __shared__ __attribute__((aligned(16))) float2 split_lds[];
  float* const raw = reinterpret_cast<float*>(split_lds);
  float2* const mixed = split_lds + off_mixed;
  float2* const lutS = split_lds + off_lut;

  const unsigned tid = threadIdx.x, g = blockIdx.y;
  const unsigned m0 = blockIdx.x * TO;
  const unsigned nout = min(TO, a.M - m0);
  const int p_first = (int)(a.pos + m0 * R);
  const int k_lo = p_first - (int)K;
  const int k_hi = p_first + (int)((nout - 1) * R) - 1;
  const unsigned Wt = (unsigned)(k_hi - k_lo + 1);
  const elem_t* __restrict__ x = static_cast<const elem_t*>(a.in) + uniform_u64((size_t)g * a.in_stride);
  const float* __restrict__ h = static_cast<const float*>(a.hist) + (size_t)g * K;

  // 1. the raw window, once for all bands: four samples a load, a float each in LDS
  {
    const int k_al = k_lo & ~3;
    const int nquads = (k_hi - k_al + 4) >> 2;
    const quad_t* __restrict__ xq = reinterpret_cast<const quad_t*>(x);
    for (int u = (int)tid; u < nquads; u += NT)
    {
      const int ka = k_al + 4 * u;
      if (ka >= 0 && ka + 3 < (int)a.N)
      {
        float s[4];
        IN::unpack(xq[ka >> 2], s);
        // (all four are wanted here: left to itself the compiler sinks the load into the conditions below and
        // splits it into smaller loads)
        asm("" : "+v"(s[0]), "+v"(s[1]), "+v"(s[2]), "+v"(s[3]));
        if (ka >= k_lo && ka + 3 <= k_hi)
        {
#pragma unroll
          for (int e = 0; e < 4; e++)
            raw[ka + e - k_lo] = s[e];
        }
        else
        {
#pragma unroll
          for (int e = 0; e < 4; e++)
            if (ka + e >= k_lo && ka + e <= k_hi)
              raw[ka + e - k_lo] = s[e];
        }
      }
      else
      {
        for (int kk = ka; kk <= ka + 3; kk++)
          if (kk >= k_lo && kk <= k_hi) // (k_hi < N, as in k_split)
            raw[kk - k_lo] = kk < 0 ? h[(int)K + kk] : IN::one(x, (size_t)kk);
      }
    }
  }
  const float2* __restrict__ lg = a.luts + (size_t)g * a.B * T;
  for (unsigned i = tid; i < T; i += NT)
    lutS[i] = lg[i];
  const unsigned idx0 = (a.lut_k + (unsigned)p_first + tid) % T;
  const float* __restrict__ coeff = a.coeff;
  const fmd_f2v scale2 = {a.scale, a.scale};
  __syncthreads();

  for (unsigned b = 0; b < a.B; b++)
  {
    // 2. mix every window sample once, (v, +0) lut = (v lut.re, v lut.im): one packed multiply; the next band's table
    const float2* ls = lutS + (b & 1u) * T;
    unsigned idx = idx0;
    for (unsigned i = tid; i < Wt; i += NT)
    {
      const float v = raw[i];
      const float2 l = ls[idx];
      const fmd_f2v t = fmd_f2v{v, v} * fmd_f2v{l.x, l.y};
      mixed[(i & emask) * RS + (i >> E)] = make_float2(t.x, t.y);
      idx += a.lut_step;
      if (idx >= T)
        idx -= T;
    }
    if (b + 1 < a.B)
    {
      float2* ln = lutS + ((b + 1u) & 1u) * T;
      for (unsigned i = tid; i < T; i += NT)
        ln[i] = lg[(size_t)(b + 1) * T + i];
    }
    __syncthreads();
    // 3. one lane per output
    if (tid < nout)
      split_taps<CT, CT ? KT : 0>(mixed + tid * (R >> E), coeff, K, emask, RS, E, scale2,
                                  a.out + ((size_t)g * a.B + b) * a.out_stride + m0 + tid);
    __syncthreads();
  }
}

/* k_split_roll for a real capture: float history */
template <class IN>
__global__ __launch_bounds__(256) void k_split_roll_real(const void* in, size_t in_stride, unsigned N,
                                                         const float* __restrict__ hist_in,
                                                         float* __restrict__ hist_out, unsigned K)
{
  typedef typename IN::elem elem_t;
  const unsigned g = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
  if (i >= K)
    return;
  const elem_t* __restrict__ x = static_cast<const elem_t*>(in) + (size_t)g * in_stride;
  const unsigned keep = N < K ? K - N : 0u;
  hist_out[(size_t)g * K + i] = i < keep ? hist_in[(size_t)g * K + i + N] : IN::one(x, (size_t)(N + i - K));
}

/* The real forms live in a translation unit of their own, fmd_split_real.hip: it instantiates them and holds the two
 * launches below.  fmd_batch.hip's object keeps the kernels it had (tests/test_call_trace_cpu.py links that object
 * alone against a recording double of the runtime and pins its kernel list), so there the two are weak references: in
 * the library they are always present, and a program that links fmd_batch.o without fmd_split_real.o gets an error
 * from fmd_split_create_real, never another kernel.
 * form: 0 = generic, 4 = <.., 4, 32>, 8 = <.., 8, 64>; format: FMD_REAL_*. */
__attribute__((weak, visibility("hidden"))) void split_real_launch(int format, int form, unsigned ntiles, unsigned G,
                                                                   unsigned lds, hipStream_t stream,
                                                                   const SplitArgs& a);
__attribute__((weak, visibility("hidden"))) void split_real_roll(int format, unsigned G, unsigned K, const void* in,
                                                                 size_t in_stride, unsigned N, const float* hist_in,
                                                                 float* hist_out, hipStream_t stream);

} // namespace fmd
