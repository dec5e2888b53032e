/*
 * fmd_k_chan.hip.h -- the polyphase channeliser's kernels (fmd_chan_*, include/fmd.h): every wideband capture filtered
 * ONCE into its N branch sums per output time, and the B wanted bins of the capture taken out of them by a matrix
 * product on the matrix cores.  Rows are channel IQ at fs / D, what a FMD_IN_CIQ_F32 call reads.  DESIGN.md section
 * 9.16.
 *
 * k_chan: one workgroup = one capture x one tile of kChanTile = 32 consecutive output times, for ALL B rows.
 *   1. The tile's raw window -- 31 D + K input samples, the carried history in front of a call's first ones -- is
 *      converted (ChanInF32 / U8 / S8 / S16, two samples per load where both lie in the call) and staged in LDS once,
 *      with the K taps beside it.
 *   2. Branch sums on the VALU: U[r][t] = sum over the taps j = j0, j0 + N, ... <= K of c[j] x[q_t - j], j0 the tap
 *      with (q_t - j0) = r (mod N) -- j ascending, one fma per tap and part, from +0.  The lanes of a wave walk r, so
 *      they read consecutive window samples and consecutive taps (conflict-free), and write U at a row stride of 33
 *      floats (conflict-free again).  Real and imaginary parts lie in two planes, 32 banks apart.
 *   3. The bins: Y[2 B x 32] = A[2 B x 2 N] U[2 N x 32] in real arithmetic on v_mfma_f32_32x32x2_f32, whose result is
 *      bit for bit an fma chain in k order (tests/test_gpu_chan_shapes.py holds the device's rows to a numpy model of
 *      these chains in bits: 5, 16, 17, 33, 37 and 70 rows a capture; N = 2, 3, 4, 5, 8, 9, 16, 24, 64, 192, 255, 256,
 *      real 2, 3, 5, 24, 192, 511).  Row 2 b of A is (Wre[0], -Wim[0], Wre[1], ...), row 2 b + 1 is (Wim[0],
 *      Wre[0], ...), W[r] = exp(+2 pi i s_b r / N) from the host's table (rounded once from double); k = 2 r + part.
 *      A wave owns blocks of 32 rows of A (16 rows of the channeliser); the chain runs in two independent halves, r in
 *      [0, N / 2) and [N / 2, N), that are added at the end -- the same form for every B, call size and tile, so a
 *      row's bits depend on nothing but its capture, its shift and the parameters.  A's operands come from global
 *      memory in the order the lanes want them (256 contiguous bytes per step), U's from LDS.
 *   4. (half0 + half1) * (2 out_scale); neighbouring lanes swap one sample so that every lane stores two consecutive
 *      times of one row: 16-byte stores (8 bytes for the odd last sample of a call).
 * k_chan_roll: the raw history of the next call into the other of two buffers, as the splitter's.
 * No scratch; nothing depends on the grid.
 *
 * Rows of 16-bit integers (FMD_CIQ_S16, template argument S16): step 4 converts the two samples a lane holds with
 * fmd_f32_to_mpx16 and stores 8 bytes (4 for the odd last sample of a call); everything in front of it is the float
 * form's, so the integers are the conversion of exactly the floats the float call stores.
 *
 * k_chan_real / k_chan_roll_real: a real-sampled capture (fmd_chan_create_real, FMD_REAL_*), x[q] = (v[q], +0): the
 * complex kernel with the terms that are zeros deleted.
 *   1. The raw window holds one float a sample (ChanInRealF32 / S8 / S16: four samples per load where all four lie in
 *      the call, the history or single loads at the edges).
 *   2. One plane of branch sums, U[N + 1][33], one fma per tap; row N is the +0 of a padded step.
 *   3. Y[2 B x 32] = A[2 B x N] U[N x 32]: one MFMA carries two branches, lanes 0-31 the lower k, lanes 32-63 the upper
 *      one.  The chain is the complex kernel's without its Im U products: one accumulator over r in [0, N / 2)
 *      ascending, a second over [N / 2, N) (for odd N branch N - 1 comes last on it, where the complex kernel has it);
 *      a half of odd length ends with a padded k: A = U = +0.  Row 2 b of A is Wre[r], row 2 b + 1 is Wim[r], a host
 *      table of its own in the order the lanes want it (chan_real_steps).
 *   4. As above, both row formats.
 *   Nothing in 2 and 3 assumes N <= 256 threads' worth of branches: the real form takes N up to 512.
 */
#pragma once

namespace fmd
{

constexpr int kChanThreads = 256;
constexpr unsigned kChanTile = 32;          // output times per workgroup: the columns of one MFMA tile
constexpr unsigned kChanUStride = 33;       // floats per branch r in a plane of U
constexpr unsigned kChanLdsBytes = 160 * 1024;

/* Where a tile's LDS regions lie (in floats), from (N, D, K) alone -- host and kernel compute the same. */
struct ChanGeom
{
  unsigned off_taps; // raw window: float2 [31 D + K] from 0
  unsigned off_qm;   // q mod N of the tile's 32 output times
  unsigned off_ure;  // U, real parts [N][33]
  unsigned off_uim;  // U, imaginary parts: 32 banks off the real plane
  unsigned total;
};
__host__ __device__ constexpr ChanGeom chan_geom(unsigned N, unsigned D, unsigned K)
{
  ChanGeom g{};
  const unsigned W = (kChanTile - 1) * D + K;
  g.off_taps = 2 * W;
  g.off_qm = g.off_taps + ((K + 1 + 3) & ~3u);
  g.off_ure = g.off_qm + kChanTile;
  unsigned plane = N * kChanUStride;
  while (plane % 64 != 32)
    plane++;
  g.off_uim = g.off_ure + plane;
  g.total = g.off_uim + N * kChanUStride;
  return g;
}

/* The real form's regions (in floats): one float a window sample, one plane of U with a row of zeros behind it. */
struct ChanRealGeom
{
  unsigned off_taps; // raw window: float [31 D + K] from 0
  unsigned off_qm;
  unsigned off_u;    // U [N + 1][33]; row N = +0, the operand of a padded step
  unsigned total;
};
__host__ __device__ constexpr ChanRealGeom chan_real_geom(unsigned N, unsigned D, unsigned K)
{
  ChanRealGeom g{};
  const unsigned W = (kChanTile - 1) * D + K;
  g.off_taps = (W + 3) & ~3u;
  g.off_qm = g.off_taps + ((K + 1 + 3) & ~3u);
  g.off_u = g.off_qm + kChanTile;
  g.total = g.off_u + (N + 1) * kChanUStride;
  return g;
}

/* The real form's MFMA steps, two branches each: s0 for r in [0, N / 2), s1 for [N / 2, N); an odd half pads its last
 * step.  The table of one row block is [s0 + s1][2][32] floats. */
struct ChanRealSteps
{
  unsigned s0, s1;
};
__host__ __device__ constexpr ChanRealSteps chan_real_steps(unsigned N)
{
  return ChanRealSteps{(N / 2 + 1) / 2, (N - N / 2 + 1) / 2};
}

/* rows of A per capture: blocks of 32 real rows = 16 rows of the channeliser */
__host__ __device__ constexpr unsigned chan_row_blocks(unsigned B)
{
  return (2 * B + 31) / 32;
}

struct ChanArgs
{
  const void* in;      // capture g at in + g * in_stride elements
  size_t in_stride;
  const float2* hist;  // [G][K]: x[q0 - K .. q0) of every capture, converted (a real channeliser: float [G][K])
  const float* atab;   // [G][row block][N][2][32]: the operand of lane l at step r is atab[.. + r * 64 + l]
                       // (a real channeliser: [G][row block][s0 + s1][2][32], chan_real_steps)
  const float* coeff;  // c[0 .. K + 1], taps c[1 .. K]
  float2* out;         // row r at out + r * out_stride (S16 rows: 4 bytes a sample behind the same pointer)
  size_t out_stride;
  unsigned n_in;       // input samples of the call
  unsigned B;          // rows per capture
  unsigned pos;        // the call's first output sits on input sample pos (q0 + pos is a multiple of D)
  unsigned M;          // outputs of the call
  unsigned q0_mod;     // q0 mod N
  float scale2;        // 2 out_scale
  unsigned N, D, K;
};

/* Input formats: a lane loads two IQ samples at a time, converted as the decoder converts FMD_IQ_*. */
struct ChanInF32
{
  typedef float2 elem;
  typedef uint4 pair;
  static __device__ __forceinline__ float2 one(const elem* x, size_t k) { return x[k]; }
  static __device__ __forceinline__ void unpack(const pair& v, float2& a, float2& b)
  {
    a = make_float2(__uint_as_float(v.x), __uint_as_float(v.y));
    b = make_float2(__uint_as_float(v.z), __uint_as_float(v.w));
  }
};
struct ChanInU8
{
  typedef uchar2 elem;
  typedef unsigned pair;
  static __device__ __forceinline__ float2 one(const elem* x, size_t k)
  {
    const uchar2 b = x[k];
    return make_float2(fmd_u8_to_f32(b.x), fmd_u8_to_f32(b.y));
  }
  static __device__ __forceinline__ void unpack(const pair& v, float2& a, float2& b)
  {
    a = make_float2(fmd_u8_to_f32(v & 0xffu), fmd_u8_to_f32((v >> 8) & 0xffu));
    b = make_float2(fmd_u8_to_f32((v >> 16) & 0xffu), fmd_u8_to_f32(v >> 24));
  }
};
struct ChanInS8
{
  typedef char2 elem;
  typedef unsigned pair;
  static __device__ __forceinline__ float2 one(const elem* x, size_t k)
  {
    const char2 b = x[k];
    return make_float2(fmd_s8_to_f32((signed char)b.x), fmd_s8_to_f32((signed char)b.y));
  }
  static __device__ __forceinline__ void unpack(const pair& v, float2& a, float2& b)
  { // shift the byte to the top, then an arithmetic shift back: sign extension
    a = make_float2(fmd_s8_to_f32((int)(v << 24) >> 24), fmd_s8_to_f32((int)(v << 16) >> 24));
    b = make_float2(fmd_s8_to_f32((int)(v << 8) >> 24), fmd_s8_to_f32((int)v >> 24));
  }
};
struct ChanInS16
{
  typedef short2 elem;
  typedef uint2 pair;
  static __device__ __forceinline__ float2 one(const elem* x, size_t k)
  {
    const short2 s = x[k];
    return make_float2(fmd_s16_to_f32(s.x), fmd_s16_to_f32(s.y));
  }
  static __device__ __forceinline__ void unpack(const pair& v, float2& a, float2& b)
  {
    a = make_float2(fmd_s16_to_f32((int)(v.x << 16) >> 16), fmd_s16_to_f32((int)v.x >> 16));
    b = make_float2(fmd_s16_to_f32((int)(v.y << 16) >> 16), fmd_s16_to_f32((int)v.y >> 16));
  }
};

/* Real-sampled input (FMD_REAL_*): one element per sample, converted like the I part of the matching FMD_IQ_*; a
 * lane loads four samples at a time (the call's pointer and capture stride are multiples of four samples). */
struct ChanInRealF32
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
struct ChanInRealS8
{
  typedef signed char elem;
  typedef unsigned quad;
  static __device__ __forceinline__ float one(const elem* x, size_t k) { return fmd_s8_to_f32(x[k]); }
  static __device__ __forceinline__ void unpack(const quad& v, float (&s)[4])
  {
    s[0] = fmd_s8_to_f32((int)(v << 24) >> 24);
    s[1] = fmd_s8_to_f32((int)(v << 16) >> 24);
    s[2] = fmd_s8_to_f32((int)(v << 8) >> 24);
    s[3] = fmd_s8_to_f32((int)v >> 24);
  }
};
struct ChanInRealS16
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

typedef float chan_f16v __attribute__((ext_vector_type(16)));

/* Two consecutive samples of a row as FMD_CIQ_S16: fmd_f32_to_mpx16 of each part, re in the low half of a word.  o:
 * the first sample's word (8-byte aligned: the row stride is a multiple of 4 samples, the time is even). */
__device__ __forceinline__ void chan_store_s16(unsigned* o, const float4& two, bool both)
{
  const unsigned w0 = ((unsigned)fmd_f32_to_mpx16(two.x) & 0xffffu) | ((unsigned)fmd_f32_to_mpx16(two.y) << 16);
  const unsigned w1 = ((unsigned)fmd_f32_to_mpx16(two.z) & 0xffffu) | ((unsigned)fmd_f32_to_mpx16(two.w) << 16);
  if (both)
    *reinterpret_cast<uint2*>(o) = make_uint2(w0, w1);
  else
    *o = w0;
}

/* Step 4 of the kernels (k_chan keeps its float form in its body, as it was): the block's accumulators to the rows. */
template <bool S16>
__device__ __forceinline__ void chan_store_block(const chan_f16v& acc0, const chan_f16v& acc1, const ChanArgs& a,
                                                 unsigned g, unsigned mb, unsigned col, unsigned hi, unsigned m0,
                                                 unsigned nout)
{
  const unsigned odd = col & 1u, tcol = col & ~1u;
#pragma unroll
  for (unsigned v = 0; v < 4; v++)
  {
    const float r0 = (acc0[4 * v] + acc1[4 * v]) * a.scale2;
    const float i0 = (acc0[4 * v + 1] + acc1[4 * v + 1]) * a.scale2;
    const float r1 = (acc0[4 * v + 2] + acc1[4 * v + 2]) * a.scale2;
    const float i1 = (acc0[4 * v + 3] + acc1[4 * v + 3]) * a.scale2;
    const float sr = __shfl_xor(odd ? r0 : r1, 1), si = __shfl_xor(odd ? i0 : i1, 1);
    const unsigned b = mb * 16 + 4 * v + 2 * hi + odd;
    if (b < a.B && tcol < nout)
    {
      const size_t at = ((size_t)g * a.B + b) * a.out_stride + m0 + tcol;
      const float4 two = odd ? make_float4(sr, si, r1, i1) : make_float4(r0, i0, sr, si);
      if constexpr (S16)
        chan_store_s16(reinterpret_cast<unsigned*>(a.out) + at, two, tcol + 1 < nout);
      else if (tcol + 1 < nout)
        *reinterpret_cast<float4*>(a.out + at) = two;
      else
        a.out[at] = make_float2(two.x, two.y);
    }
  }
}

template <class IN, bool S16 = false>
__global__ __launch_bounds__(kChanThreads) void k_chan(const ChanArgs a)
{
  typedef typename IN::pair pair_t;
  typedef typename IN::elem elem_t;
  constexpr int NT = kChanThreads;
  constexpr unsigned US = kChanUStride;
  const unsigned N = a.N, D = a.D, K = a.K;
  const ChanGeom cg = chan_geom(N, D, K);
  extern __shared__ __attribute__((aligned(16))) float chan_lds[];
  float2* const raw = reinterpret_cast<float2*>(chan_lds);
  float* const taps = chan_lds + cg.off_taps;
  unsigned* const qm = reinterpret_cast<unsigned*>(chan_lds + cg.off_qm);
  float* const ure = chan_lds + cg.off_ure;
  float* const uim = chan_lds + cg.off_uim;

  const unsigned tid = threadIdx.x, g = blockIdx.y;
  const unsigned m0 = blockIdx.x * kChanTile;
  const unsigned nout = min(kChanTile, a.M - m0);
  const int p_first = (int)(a.pos + m0 * D);      // input sample of the tile's first output
  const int k_lo = p_first - (int)K;              // the window: samples k_lo .. k_hi of the call (k < 0: history)
  const int k_hi = p_first + (int)((nout - 1) * D) - 1;
  const elem_t* __restrict__ x = static_cast<const elem_t*>(a.in) + (size_t)g * a.in_stride;
  const float2* __restrict__ h = a.hist + (size_t)g * K;

  // 1. the raw window, the taps and q mod N of every output time
  {
    const int k_al = k_lo & ~1;
    const int npairs = (k_hi - k_al + 2) >> 1;
    const pair_t* __restrict__ xp = reinterpret_cast<const pair_t*>(x);
    for (int u = (int)tid; u < npairs; u += NT)
    {
      const int ka = k_al + 2 * u;
      if (ka >= 0 && ka + 1 < (int)a.n_in)
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
          if (kk >= k_lo && kk <= k_hi) // (k_hi < n_in: an output needs nothing behind the sample in front of it)
            raw[kk - k_lo] = kk < 0 ? h[(int)K + kk] : IN::one(x, (size_t)kk);
      }
    }
    for (unsigned i = tid; i <= K; i += NT)
      taps[i] = a.coeff[i];
    if (tid < kChanTile)
      qm[tid] = (a.q0_mod + ((unsigned)p_first + tid * D) % N) % N;
  }
  __syncthreads();

  // 2. the branch sums: item e = t N + r goes to thread e mod 256, so a wave's lanes walk r
  {
    unsigned t = tid / N, r = tid - t * N;
    const unsigned dt = (unsigned)NT / N, dr = (unsigned)NT - dt * N;
    while (t < nout)
    {
      int j = (int)qm[t] - (int)r; // the first tap on branch r: (q - j) = r (mod N), 1 <= j <= N
      if (j <= 0)
        j += (int)N;
      const float2* w = raw + t * D + K; // x[q_t - j] = w[-j]
      float re = 0.0f, im = 0.0f;
      for (; j <= (int)K; j += (int)N)
      {
        const float c = taps[j];
        const float2 s = w[-j];
        re = __builtin_fmaf(c, s.x, re);
        im = __builtin_fmaf(c, s.y, im);
      }
      ure[r * US + t] = re;
      uim[r * US + t] = im;
      r += dr;
      t += dt;
      if (r >= N)
      {
        r -= N;
        t++;
      }
    }
  }
  __syncthreads();

  // 3. the bins: a wave per block of 32 rows of A, two half chains
  const unsigned lane = tid & 63u, wave = tid >> 6;
  const unsigned col = lane & 31u, hi = lane >> 5;
  const unsigned nmb = chan_row_blocks(a.B);
  const unsigned Nh = N >> 1;
  const float* __restrict__ up = (hi ? uim : ure) + col;
  for (unsigned mb = wave; mb < nmb; mb += NT / 64)
  {
    const float* __restrict__ ap = a.atab + ((size_t)g * nmb + mb) * N * 64 + lane;
    const float* __restrict__ ap1 = ap + (size_t)Nh * 64;
    const float* __restrict__ up1 = up + Nh * US;
    chan_f16v acc0 = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    chan_f16v acc1 = acc0;
    // groups of GS steps; the table operands of the next group are fetched (index clamped, always inside the block's
    // table) while this group's products run
    constexpr unsigned GS = 8;
    float na0[GS], na1[GS];
#pragma unroll
    for (unsigned u = 0; u < GS; u++)
    {
      const unsigned r = min(u, Nh - 1);
      na0[u] = ap[(size_t)r * 64];
      na1[u] = ap1[(size_t)r * 64];
    }
    for (unsigned r0 = 0; r0 < Nh; r0 += GS)
    {
      float a0[GS], a1[GS], b0[GS], b1[GS];
#pragma unroll
      for (unsigned u = 0; u < GS; u++)
      {
        a0[u] = na0[u];
        a1[u] = na1[u];
        const unsigned rn = min(r0 + GS + u, Nh - 1), r = min(r0 + u, Nh - 1);
        na0[u] = ap[(size_t)rn * 64];
        na1[u] = ap1[(size_t)rn * 64];
        b0[u] = up[r * US];
        b1[u] = up1[r * US];
      }
#pragma unroll
      for (unsigned u = 0; u < GS; u++)
        if (r0 + u < Nh)
        {
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], b0[u], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], b1[u], acc1, 0, 0, 0);
        }
    }
    if (N & 1u)
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[(size_t)(N - 1) * 64], up[(N - 1) * US], acc1, 0, 0, 0);

    // 4. lane (col, hi) holds, in registers 4 v .. 4 v + 3, rows b0 = 16 mb + 4 v + 2 hi and b0 + 1 at time col (re,
    // im each).  Even columns keep b0 and take the neighbour's b0, odd ones keep b0 + 1: two consecutive times a lane.
    if constexpr (S16)
    {
      chan_store_block<true>(acc0, acc1, a, g, mb, col, hi, m0, nout);
      continue;
    }
    const unsigned odd = col & 1u, tcol = col & ~1u;
#pragma unroll
    for (unsigned v = 0; v < 4; v++)
    {
      const float r0 = (acc0[4 * v] + acc1[4 * v]) * a.scale2;
      const float i0 = (acc0[4 * v + 1] + acc1[4 * v + 1]) * a.scale2;
      const float r1 = (acc0[4 * v + 2] + acc1[4 * v + 2]) * a.scale2;
      const float i1 = (acc0[4 * v + 3] + acc1[4 * v + 3]) * a.scale2;
      const float sr = __shfl_xor(odd ? r0 : r1, 1), si = __shfl_xor(odd ? i0 : i1, 1);
      const unsigned b = mb * 16 + 4 * v + 2 * hi + odd;
      if (b < a.B && tcol < nout)
      {
        float2* o = a.out + ((size_t)g * a.B + b) * a.out_stride + m0 + tcol;
        const float4 two = odd ? make_float4(sr, si, r1, i1) : make_float4(r0, i0, sr, si);
        if (tcol + 1 < nout)
          *reinterpret_cast<float4*>(o) = two;
        else
          *o = make_float2(two.x, two.y);
      }
    }
  }
}

/* k_chan for a real capture (the file's head): a.hist float [G][K], a.in / a.in_stride / a.n_in in real samples,
 * a.atab the real table. */
template <class IN, bool S16>
__global__ __launch_bounds__(kChanThreads) void k_chan_real(const ChanArgs a)
{
  typedef typename IN::quad quad_t;
  typedef typename IN::elem elem_t;
  constexpr int NT = kChanThreads;
  constexpr unsigned US = kChanUStride;
  const unsigned N = a.N, D = a.D, K = a.K;
  const ChanRealGeom cg = chan_real_geom(N, D, K);
  extern __shared__ __attribute__((aligned(16))) float chan_lds[];
  float* const raw = chan_lds;
  float* const taps = chan_lds + cg.off_taps;
  unsigned* const qm = reinterpret_cast<unsigned*>(chan_lds + cg.off_qm);
  float* const us = chan_lds + cg.off_u;

  const unsigned tid = threadIdx.x, g = blockIdx.y;
  const unsigned m0 = blockIdx.x * kChanTile;
  const unsigned nout = min(kChanTile, a.M - m0);
  const int p_first = (int)(a.pos + m0 * D);
  const int k_lo = p_first - (int)K;
  const int k_hi = p_first + (int)((nout - 1) * D) - 1;
  const elem_t* __restrict__ x = static_cast<const elem_t*>(a.in) + (size_t)g * a.in_stride;
  const float* __restrict__ h = reinterpret_cast<const float*>(a.hist) + (size_t)g * K;

  // 1. the raw window: four samples a load, a float each in LDS; the taps, q mod N, the zeros of a padded step
  {
    const int k_al = k_lo & ~3;
    const int nquads = (k_hi - k_al + 4) >> 2;
    const quad_t* __restrict__ xq = reinterpret_cast<const quad_t*>(x);
    for (int u = (int)tid; u < nquads; u += NT)
    {
      const int ka = k_al + 4 * u;
      if (ka >= 0 && ka + 3 < (int)a.n_in)
      {
        float s[4];
        IN::unpack(xq[ka >> 2], s);
#pragma unroll
        for (int e = 0; e < 4; e++)
          if (ka + e >= k_lo && ka + e <= k_hi)
            raw[ka + e - k_lo] = s[e];
      }
      else
      {
        for (int kk = ka; kk <= ka + 3; kk++)
          if (kk >= k_lo && kk <= k_hi) // (k_hi < n_in, as in k_chan)
            raw[kk - k_lo] = kk < 0 ? h[(int)K + kk] : IN::one(x, (size_t)kk);
      }
    }
    for (unsigned i = tid; i <= K; i += NT)
      taps[i] = a.coeff[i];
    if (tid < kChanTile)
      qm[tid] = (a.q0_mod + ((unsigned)p_first + tid * D) % N) % N;
    if (tid < US)
      us[N * US + tid] = 0.0f;
  }
  __syncthreads();

  // 2. the branch sums: item e = t N + r goes to thread e mod 256 (N above 256: a thread's items are 256 apart, so
  // dt = 0 and r wraps at most once a step)
  {
    unsigned t = tid / N, r = tid - t * N;
    const unsigned dt = (unsigned)NT / N, dr = (unsigned)NT - dt * N;
    while (t < nout)
    {
      int j = (int)qm[t] - (int)r;
      if (j <= 0)
        j += (int)N;
      const float* w = raw + t * D + K; // x[q_t - j] = w[-j]
      float re = 0.0f;
      for (; j <= (int)K; j += (int)N)
        re = __builtin_fmaf(taps[j], w[-j], re);
      us[r * US + t] = re;
      r += dr;
      t += dt;
      if (r >= N)
      {
        r -= N;
        t++;
      }
    }
  }
  __syncthreads();

  // 3. the bins: lane (col, hi) supplies branch 2 s + hi of each half at step s; behind a half's end the row of zeros
  const unsigned lane = tid & 63u, wave = tid >> 6;
  const unsigned col = lane & 31u, hi = lane >> 5;
  const unsigned nmb = chan_row_blocks(a.B);
  const unsigned Nh = N >> 1, L1 = N - Nh;
  const ChanRealSteps st = chan_real_steps(N);
  const float* __restrict__ up = us + col;
  for (unsigned mb = wave; mb < nmb; mb += NT / 64)
  {
    const float* __restrict__ ap = a.atab + ((size_t)g * nmb + mb) * (st.s0 + st.s1) * 64 + lane;
    const float* __restrict__ ap1 = ap + (size_t)st.s0 * 64;
    chan_f16v acc0 = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    chan_f16v acc1 = acc0;
    constexpr unsigned GS = 8;
    float na0[GS], na1[GS];
#pragma unroll
    for (unsigned u = 0; u < GS; u++)
    {
      na0[u] = ap[(size_t)min(u, st.s0 - 1) * 64];
      na1[u] = ap1[(size_t)min(u, st.s1 - 1) * 64];
    }
    for (unsigned s0 = 0; s0 < st.s1; s0 += GS) // (s1 >= s0 >= 1)
    {
      float a0[GS], a1[GS], b0[GS], b1[GS];
#pragma unroll
      for (unsigned u = 0; u < GS; u++)
      {
        a0[u] = na0[u];
        a1[u] = na1[u];
        const unsigned sn = s0 + GS + u, s = s0 + u;
        na0[u] = ap[(size_t)min(sn, st.s0 - 1) * 64];
        na1[u] = ap1[(size_t)min(sn, st.s1 - 1) * 64];
        const unsigned i0 = 2 * min(s, st.s0 - 1) + hi, i1 = 2 * min(s, st.s1 - 1) + hi;
        b0[u] = up[(i0 < Nh ? i0 : N) * US];
        b1[u] = up[(i1 < L1 ? Nh + i1 : N) * US];
      }
#pragma unroll
      for (unsigned u = 0; u < GS; u++)
      {
        if (s0 + u < st.s0)
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], b0[u], acc0, 0, 0, 0);
        if (s0 + u < st.s1)
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], b1[u], acc1, 0, 0, 0);
      }
    }
    chan_store_block<S16>(acc0, acc1, a, g, mb, col, hi, m0, nout);
  }
}

/* The next call's raw history: ho[i] = x[q0 + n - K + i], from the old history where the call was shorter than K. */
template <class IN>
__global__ __launch_bounds__(256) void k_chan_roll(const void* in, size_t in_stride, unsigned n,
                                                   const float2* __restrict__ hist_in, float2* __restrict__ hist_out,
                                                   unsigned K)
{
  typedef typename IN::elem elem_t;
  const unsigned g = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
  if (i >= K)
    return;
  const elem_t* __restrict__ x = static_cast<const elem_t*>(in) + (size_t)g * in_stride;
  const unsigned keep = n < K ? K - n : 0u;
  hist_out[(size_t)g * K + i] = i < keep ? hist_in[(size_t)g * K + i + n] : IN::one(x, (size_t)(n + i - K));
}

template <class IN>
__global__ __launch_bounds__(256) void k_chan_roll_real(const void* in, size_t in_stride, unsigned n,
                                                        const float* __restrict__ hist_in,
                                                        float* __restrict__ hist_out, unsigned K)
{
  typedef typename IN::elem elem_t;
  const unsigned g = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
  if (i >= K)
    return;
  const elem_t* __restrict__ x = static_cast<const elem_t*>(in) + (size_t)g * in_stride;
  const unsigned keep = n < K ? K - n : 0u;
  hist_out[(size_t)g * K + i] = i < keep ? hist_in[(size_t)g * K + i + n] : IN::one(x, (size_t)(n + i - K));
}

/* The kernels live in a translation unit of their own, fmd_chan.hip: it instantiates them and holds the three
 * functions below.  fmd_batch.hip's object keeps the kernels it had, so there the three are weak references: in the
 * library they are always present, and a program that links fmd_batch.o without fmd_chan.o gets an error from
 * fmd_chan_create, never another kernel.  format: FMD_IQ_*, or FMD_REAL_* for the real form's kernels; s16: FMD_CIQ_S16
 * rows. */
__attribute__((weak, visibility("hidden"))) int chan_prepare(unsigned lds_bytes); // a hipError_t
__attribute__((weak, visibility("hidden"))) void chan_launch(int format, bool s16, unsigned ntiles, unsigned G,
                                                             unsigned lds, hipStream_t stream, const ChanArgs& a);
__attribute__((weak, visibility("hidden"))) void chan_roll(int format, unsigned G, unsigned K, const void* in,
                                                           size_t in_stride, unsigned n, const float2* hist_in,
                                                           float2* hist_out, hipStream_t stream);

} // namespace fmd
