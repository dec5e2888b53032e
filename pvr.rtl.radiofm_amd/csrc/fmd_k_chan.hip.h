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
 *      bit for bit an fma chain in k order.  Row 2 b of A is (Wre[0], -Wim[0], Wre[1], ...), row 2 b + 1 is (Wim[0],
 *      Wre[0], ...), W[r] = exp(+2 pi i s_b r / N) from the host's table (rounded once from double); k = 2 r + part.
 *      A wave owns blocks of 32 rows of A (16 rows of the channeliser); the chain runs in two independent halves, r in
 *      [0, N / 2) and [N / 2, N), that are added at the end -- the same form for every B, call size and tile, so a
 *      row's bits depend on nothing but its capture, its shift and the parameters.  A's operands come from global
 *      memory in the order the lanes want them (256 contiguous bytes per step), U's from LDS.
 *   4. (half0 + half1) * (2 out_scale); neighbouring lanes swap one sample so that every lane stores two consecutive
 *      times of one row: 16-byte stores (8 bytes for the odd last sample of a call).
 * k_chan_roll: the raw history of the next call into the other of two buffers, as the splitter's.
 * No scratch; nothing depends on the grid.
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

/* rows of A per capture: blocks of 32 real rows = 16 rows of the channeliser */
__host__ __device__ constexpr unsigned chan_row_blocks(unsigned B)
{
  return (2 * B + 31) / 32;
}

struct ChanArgs
{
  const void* in;      // capture g at in + g * in_stride elements
  size_t in_stride;
  const float2* hist;  // [G][K]: x[q0 - K .. q0) of every capture, converted
  const float* atab;   // [G][row block][N][2][32]: the operand of lane l at step r is atab[.. + r * 64 + l]
  const float* coeff;  // c[0 .. K + 1], taps c[1 .. K]
  float2* out;         // row r at out + r * out_stride
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

typedef float chan_f16v __attribute__((ext_vector_type(16)));

template <class IN>
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

/* The kernels live in a translation unit of their own, fmd_chan.hip: it instantiates them and holds the three
 * functions below.  fmd_batch.hip's object keeps the kernels it had, so there the three are weak references: in the
 * library they are always present, and a program that links fmd_batch.o without fmd_chan.o gets an error from
 * fmd_chan_create, never another kernel.  format: FMD_IQ_*. */
__attribute__((weak, visibility("hidden"))) int chan_prepare(unsigned lds_bytes); // a hipError_t
__attribute__((weak, visibility("hidden"))) void chan_launch(int format, unsigned ntiles, unsigned G, unsigned lds,
                                                             hipStream_t stream, const ChanArgs& a);
__attribute__((weak, visibility("hidden"))) void chan_roll(int format, unsigned G, unsigned K, const void* in,
                                                           size_t in_stride, unsigned n, const float2* hist_in,
                                                           float2* hist_out, hipStream_t stream);

} // namespace fmd
