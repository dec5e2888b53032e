/*
 * fmd_k_rds.hip.h -- RDS branch: half-band decimators (k_halfband*, k_halfband_chain), the ring-buffer FIR filters
 * (k_ring_fir, k_ring_fir4: RDS low-pass, matched filter, audio low-pass), RDS PLL and bit / block recovery
 * (k_rds_pll, k_rds_bits).
 * Part of fmd_kernels.hip.h (layout, numerics contract and citations: see there and fmd_k_common.hip.h).
 */
#pragma once

#include "fmd_k_common.hip.h"

namespace fmd
{

/* ------------------------------------------------------------------------------------------ */
/* K3: CHalfBandDecimateBy2::DecBy2 (DownConvert.cpp:512-550), time-parallel.  in has L-1       */
/*     history rows in front; output k reads rows 2k .. 2k+L-1.  Tap 0 is counted twice and     */
/*     the centre tap added last, like the reference.                                           */
/* ------------------------------------------------------------------------------------------ */
struct HbCoef
{
  float c[52];
  float e[28]; // the even taps c[0], c[2], ... packed (k_halfband4 reads runs of them)
};

#ifndef FMD_HB_R
#define FMD_HB_R 4
#endif
constexpr int HB_R = FMD_HB_R; // outputs per thread: each even input row is loaded once for up to 4 outputs

__global__ __launch_bounds__(256) void k_halfband(const float2* __restrict__ in,
                                                  float2* __restrict__ out, unsigned n_out, int L,
                                                  HbCoef hc, unsigned C, unsigned CP, unsigned Hout)
{
  const unsigned c = blockIdx.x * 64 + threadIdx.x;
  // threadIdx.y is the same for all 64 lanes of a wave; saying so keeps tap/table loads scalar
  const unsigned wy = (unsigned)__builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const unsigned k0 = (blockIdx.y * blockDim.y + wy) * HB_R;
  if (c >= C || k0 >= n_out)
    return;
  const int nr = (int)min((unsigned)HB_R, n_out - k0);
  const int half = (L - 1) / 2; // index of the last even tap is 2*half' with half' = (L-1)/2
  const int mid = half;
  const float2* __restrict__ p = in + (size_t)(2 * k0) * CP + c;
  float ar[HB_R], ai[HB_R];
  // even rows e = 2*k0 + 2*u feed output r with tap j = 2*(u - r), in ascending j per output
  const int nu = half + nr; // u = 0 .. half + nr - 1
  for (int u0 = 0; u0 < nu; u0 += 4)
  {
    float2 xs[4];
#pragma unroll
    for (int q = 0; q < 4; q++) // four independent loads in flight (index clamped, not branched)
      xs[q] = p[(size_t)(2 * min(u0 + q, nu - 1)) * CP];
#pragma unroll
    for (int q = 0; q < 4; q++)
    {
      const int u = u0 + q;
      const float2 x = xs[q];
#pragma unroll
      for (int r = 0; r < HB_R; r++)
      {
        const int jh = u - r;
        if (u < nu && r < nr && jh >= 0 && jh <= half)
        {
          const float cj = hc.c[2 * jh];
          if (jh == 0)
          { // :529-530 tap 0 initialises the accumulator and is then added again in the loop
            ar[r] = x.x * cj;
            ai[r] = x.y * cj;
          }
          ar[r] = ar[r] + x.x * cj;
          ai[r] = ai[r] + x.y * cj;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < HB_R; r++)
  {
    if (r < nr)
    {
      const float2 x = p[(size_t)(2 * r + mid) * CP];
      ar[r] = ar[r] + x.x * hc.c[mid];
      ai[r] = ai[r] + x.y * hc.c[mid];
      out[(size_t)(Hout + k0 + r) * CP + c] = make_float2(ar[r], ai[r]);
    }
  }
}

/* Short blocks.  CHalfBandDecimateBy2::DecBy2 works in place (pInData == pOutData, DownConvert.cpp:
 * 480) and has two regimes below 2 (L - 1) inputs that are part of what the reference computes:
 *  - InLength < L (:519-520): nothing is filtered, the call returns InLength / 2 and the "outputs" are
 *    the first InLength / 2 INPUTS; the delay line is left alone           -> k_hb_pass, no roll
 *  - L <= InLength < 2 (L - 1): filtered as usual, but the delay line is refilled from the in / out
 *    array after the outputs were written over its front (:546-547): entry i is array element
 *    InLength - L + 1 + i, which is an OUTPUT when that index is below the output count
 *                                                                           -> k_roll_hb_mixed */
__global__ void k_hb_pass(const float2* __restrict__ in, unsigned H, float2* __restrict__ out, unsigned Hout,
                          unsigned n_out, unsigned CP)
{
  const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= CP)
    return;
  for (unsigned k = blockIdx.y; k < n_out; k += gridDim.y)
    out[(size_t)(Hout + k) * CP + c] = in[(size_t)(H + k) * CP + c];
}

/* dst rows [0, H) <- array elements n - H + r: outputs (rows Hout + idx of `outp`) below n_out, else
 * inputs (rows H + idx of `in`).  dst may be `in` (rows move towards the front: ascending order). */
__global__ void k_roll_hb_mixed(const float2* in, const float2* __restrict__ outp, float2* dst, unsigned H,
                                unsigned n, unsigned n_out, unsigned Hout, unsigned CP)
{
  const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= CP)
    return;
  for (unsigned r = 0; r < H; r++)
  {
    const unsigned idx = n - H + r;
    dst[(size_t)r * CP + c] = idx < n_out ? outp[(size_t)(Hout + idx) * CP + c] : in[(size_t)(H + idx) * CP + c];
  }
}

/* CHalfBand11TapDecimateBy2::DecBy2 (DownConvert.cpp:589-688), the first stage when the baseband
 * rate is 320 kHz or more (SetDataRate, :340-341).  Same window indexing as above with L = 11
 * (10 history rows = the class's d0..d9), but a different sum: seven products H0 x0 + H2 x2 + H4 x4 +
 * H5 x5 + H6 x6 + H8 x8 + H10 x10 added left to right as written (:596-661), the centre tap in its
 * place, no tap counted twice; InLength / 2 outputs (an odd last input is only kept as history). */
__global__ __launch_bounds__(256) void k_halfband11(const float2* __restrict__ in,
                                                    float2* __restrict__ out, unsigned n_out, HbCoef hc,
                                                    unsigned C, unsigned CP, unsigned Hout)
{
  const unsigned c = blockIdx.x * 64 + threadIdx.x;
  const unsigned wy = (unsigned)__builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const unsigned o = blockIdx.y * blockDim.y + wy;
  if (c >= C || o >= n_out)
    return;
  const float2* __restrict__ p = in + (size_t)(2 * o) * CP + c;
  const int T[7] = {0, 2, 4, 5, 6, 8, 10};
  float2 x[7];
#pragma unroll
  for (int t = 0; t < 7; t++)
    x[t] = p[(size_t)T[t] * CP];
  float ar = hc.c[0] * x[0].x, ai = hc.c[0] * x[0].y;
#pragma unroll
  for (int t = 1; t < 7; t++)
  {
    ar = ar + hc.c[T[t]] * x[t].x;
    ai = ai + hc.c[T[t]] * x[t].y;
  }
  out[(size_t)(Hout + o) * CP + c] = make_float2(ar, ai);
}

/* CCicN3DecimateBy2::DecBy2 (DownConvert.cpp:706-727): the first stage(s) at baseband rates of 5.33 MHz and more.
 * out[j] = .125 * (odd + m_Xeven + 3.0 * (m_Xodd + even)) with even = x[2j], odd = x[2j + 1], m_Xeven = x[2j - 2],
 * m_Xodd = x[2j - 1]: a window of four rows, two of them delay line (rows 0, 1 of `in`), time-parallel.  The two
 * float sums first, then double arithmetic, narrowed once -- the reference's promotions (.125 and 3.0 are double
 * literals).  InLength / 2 outputs: the host refuses odd lengths (the class reads past the block then, :701). */
__global__ __launch_bounds__(256) void k_cic3(const float2* __restrict__ in, float2* __restrict__ out, unsigned n_out,
                                              unsigned C, unsigned CP, unsigned Hout)
{
  const unsigned c = blockIdx.x * 64 + threadIdx.x;
  const unsigned wy = (unsigned)__builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const unsigned o = blockIdx.y * blockDim.y + wy;
  if (c >= C || o >= n_out)
    return;
  const float2* __restrict__ p = in + (size_t)(2 * o) * CP + c;
  const float2 xe = p[0], xo = p[CP], ev = p[(size_t)2 * CP], od = p[(size_t)3 * CP];
  const float re = (float)(.125 * ((double)(od.x + xe.x) + 3.0 * (double)(xo.x + ev.x)));
  const float im = (float)(.125 * ((double)(od.y + xe.y) + 3.0 * (double)(xo.y + ev.y)));
  out[(size_t)(Hout + o) * CP + c] = make_float2(re, im);
}

/* ------------------------------------------------------------------------------------------ */
/* K4: cFirFilter::Process(complex) / ProcessTwo (FirFilter.cpp:330-350, :387-413),            */
/*     time-parallel.  The reference walks its ring buffer from slot 0, so output i (global     */
/*     index g = g0 + i since the filter was initialised) sums ages a0, a0+1, ..., T-1, 0, ...  */
/*     with a0 = g mod T, starting from the first product (no leading zero).  in has T-1        */
/*     history rows in front (zeros after init).  I and Q taps are the same table.              */
/* ------------------------------------------------------------------------------------------ */
constexpr int RF_TI = 32; // outputs per workgroup tile

__device__ __forceinline__ float rf_mul(float k, float x) { return k * x; }
__device__ __forceinline__ float2 rf_mul(float k, float2 x) { return make_float2(k * x.x, k * x.y); }
__device__ __forceinline__ void rf_acc(float& a, float k, float x) { a += k * x; }
__device__ __forceinline__ void rf_acc(float2& a, float k, float2 x)
{
  a.x += k * x.x;
  a.y += k * x.y;
}

/* The same filter without per-term tests: thread = (channel lane, RR consecutive outputs).  Output
 * r takes the even rows u = r .. r + half (row u = input row 2*k0 + 2u) with the even taps
 * e[u - r]; so the rows u = RR-1 .. half are taken by every output, with RR taps that are
 * contiguous in e[], and only the first and last RR-1 rows by some.  Tap 0 starts the sum and is
 * added again, the centre tap comes last, like the reference.  Needs half >= RR. */
template <int RR>
__device__ __forceinline__ void hb_group(const float2* __restrict__ in, float2* __restrict__ out,
                                         unsigned k0, int half, const HbCoef& hc, unsigned c, unsigned CP,
                                         unsigned Hout)
{
  const float2* __restrict__ p = in + (size_t)(2 * k0) * CP + c;
  float2 acc[RR];
  const size_t step = (size_t)2 * CP;
#pragma unroll
  for (int u = 0; u < RR; u++) // the rows on which outputs start (u == r: tap 0, twice)
  {
    const float2 x = p[(size_t)u * step];
    acc[u] = rf_mul(hc.e[0], x);
    rf_acc(acc[u], hc.e[0], x);
#pragma unroll
    for (int r = 0; r < u; r++)
      rf_acc(acc[r], hc.e[u - r], x);
  }
#pragma unroll 4
  for (int u = RR; u <= half; u++) // every output: taps e[u], e[u-1], ..., e[u-RR+1]
  {
    const float2 x = p[(size_t)u * step];
#pragma unroll
    for (int r = 0; r < RR; r++)
      rf_acc(acc[r], hc.e[u - r], x);
  }
#pragma unroll
  for (int m = 1; m < RR; m++) // the rows behind the first output's window
  {
    const float2 x = p[(size_t)(half + m) * step];
#pragma unroll
    for (int r = m; r < RR; r++)
      rf_acc(acc[r], hc.e[half + m - r], x);
  }
#pragma unroll
  for (int r = 0; r < RR; r++)
  {
    const float2 x = p[(size_t)(2 * r + half) * CP];
    rf_acc(acc[r], hc.c[half], x);
    out[(size_t)(Hout + k0 + r) * CP + c] = acc[r];
  }
}

__global__ __launch_bounds__(256) void k_halfband4(const float2* __restrict__ in,
                                                   float2* __restrict__ out, unsigned n_out, int L,
                                                   HbCoef hc, unsigned C, unsigned CP, unsigned Hout)
{
  const unsigned c = blockIdx.x * 64 + threadIdx.x;
  const unsigned wy = (unsigned)__builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const unsigned k0 = (blockIdx.y * blockDim.y + wy) * 4;
  if (c >= C || k0 >= n_out)
    return;
  const int half = (L - 1) / 2;
  switch (min(4u, n_out - k0))
  {
    case 4: hb_group<4>(in, out, k0, half, hc, c, CP, Hout); break;
    case 3: hb_group<3>(in, out, k0, half, hc, c, CP, Hout); break;
    case 2: hb_group<2>(in, out, k0, half, hc, c, CP, Hout); break;
    default: hb_group<1>(in, out, k0, half, hc, c, CP, Hout); break;
  }
}

/* ------------------------------------------------------------------------------------------ */
/* K3': the three half-band stages of the usual chains as ONE stream (large batches).            */
/*                                                                                              */
/* Three launches of k_halfband4 move the intermediate rows through memory twice (write, read:    */
/* 0.7 GB per call at 8192 channels for 0.44 GB of input and output).  Here a workgroup owns 64  */
/* channels and a stretch of the last stage's outputs and walks it in time order; the outputs of */
/* stage 0 and stage 1 only ever exist in two LDS rings of 64 rows ([row][lane] float2).  A step  */
/* = up to 16 / 8 / 4 outputs of stage 0 / 1 / 2, a group of 4 / 2 / 1 per wave (hb_rows: the     */
/* same sums in the same order as hb_group), two barriers.  The steps of a stretch -- how far      */
/* each stage may run given what its input ring holds and what its output ring can take -- are    */
/* the same for every channel: the host lists them (HbStep).  A stretch that does not start at   */
/* the call's first output computes the 22 + 2 * 42 stage-0 outputs (+ 42 of stage 1) in front of */
/* it again; the call's first rows find the previous call's last outputs in the rings (loaded     */
/* from the history rows of the stage buffers, which the per-stage kernels keep too: the two      */
/* forms can follow each other), and the last outputs of stages 0 and 1 go to `tail1` / `tail2`, */
/* from where the chain's roll moves them into those history rows.  Stage 0's rows are fetched    */
/* a step ahead (15 rows per wave and step in registers).                                         */
/* ------------------------------------------------------------------------------------------ */
/* An entry of the RDS oscillator's table as the chain takes it: the value (x, y) and the two products of
 * CRDSDownConvert::ProcessData's complex multiplication that do not depend on the channel, -(0 y) and 0 x
 * (DownConvert.cpp:464-465 with an imaginary part of zero) -- made once per call on the host, by the same IEEE
 * multiplications. */
struct HbOsc
{
  float2 xy; // the oscillator's value
  float2 z;  // (-(0 y), 0 x)
};

/* Behind a call that wrote no mixed rows: the H rows of history the NEXT call's first half-band stage
 * finds in front of its input, should that call take a launch per stage (rows M - H .. M - 1 of
 * baseband x oscillator, as the serial stage's MIX form writes them). */
__global__ void k_mix_tail(const float2* __restrict__ br_last, const HbOsc* __restrict__ osc_last,
                           float2* __restrict__ dst, unsigned H, unsigned CP)
{
  const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= CP)
    return;
  for (unsigned r = blockIdx.y; r < H; r += gridDim.y)
  {
    const float v = br_last[(size_t)r * CP + c].x;
    const float2 o = osc_last[r].xy;
    const float zero = 0.0f;
    dst[(size_t)r * CP + c] = make_float2((v * o.x) - (zero * o.y), (v * o.y) + (zero * o.x));
  }
}

struct HbStep
{
  int a_lo, b_lo, c_lo; // the first output of stage 0 / 1 / 2 this step computes
  unsigned n;           // how many, and what else the kernel would otherwise carry in registers or fetch (HBF_*)
};
/* HbStep::n: outputs of stage 0 (0 .. 16) | stage 1 (0 .. 8) << 5 | stage 2 (0 .. 4) << 9;
 * HBF_TAIL0 / HBF_TAIL1: among them are outputs of stage 0 / 1 that belong to the next call's history;
 * HBF_LAST: the stretch's last step; bits 16 .. 21: how far a_lo of the step HBF_NSET - 1 steps ahead (the stretch's
 * last step at its end) lies in front of this one's -- the rows the kernel fetches during this step; bits 22 .. 31
 * (steps with HBF_TAIL0 / HBF_TAIL1): how many records further the stretch's HbTails lies. */
constexpr unsigned HBF_TAIL0 = 1u << 12, HBF_TAIL1 = 1u << 13, HBF_LAST = 1u << 14;
constexpr int HBF_FAR_SHIFT = 16, HBF_TAILS_SHIFT = 22;
/* Where the last outputs of stages 0 and 1 go: needed in a few steps at the end of a call only, so the kernel
 * fetches it there instead of carrying it in registers.  A copy sits behind every stretch's last step, in the place
 * of two records. */
struct HbTails
{
  float2 *tail1, *tail2;
  int first1, first2; // n0 - L1H, n1 - L2H: the first outputs of stages 0 / 1 that are history (may be negative)
  int pad0, pad1;
};
static_assert(sizeof(HbTails) == 2 * sizeof(HbStep), "the step list's header");
/* A pointer that came out of memory is a generic one to the compiler, and a store through it a FLAT instruction,
 * behind which every wait for a load is a wait for all of them: say that it points to global memory. */
typedef float HbPair __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void hb_store_global(float2* p, float2 v)
{
  HbPair x;
  x[0] = v.x;
  x[1] = v.y;
  *(__attribute__((address_space(1))) HbPair*)p = x;
}
constexpr int HBF_RING = 64; // rows per ring (power of two): >= L - 1 + two steps' outputs of the stage before
constexpr int HBF_NSET = 4;  // a stretch's list is a multiple of this many steps; the kernel reads the list (and
                             // fetches stage 0's rows) up to as many steps ahead: the host pads the list's end

/* Rows a group's window may reach past stage 0's last input row 2 H0 + n_in - 1: the group starts at output
 * n0 + 4 * 3 at most (n0 = (n_in + 1) / 2: a step without outputs for stage 0 at the end of the call) and takes rows
 * up to 2 k0 + 2 (3 + H0), so 2 n0 + 30 + 2 H0 - (2 H0 + n_in - 1) <= 32. */
constexpr int HBF_SLACK = 32;

/* The taps of the three stages as hb_rows consumes them: per stage the even taps c[0], c[2], .. c[2 HALF] and then
 * the centre tap c[HALF] -- (H0 + 2) + (H1 + 2) + (H2 + 2) floats, 45 for the longer chain, two to a scalar
 * register pair.  A packed multiplication takes either half of such a pair for both of its components (op_sel);
 * the compiler does not know that and spreads every scalar factor over a pair of its own, 90 registers for 45
 * taps, which it then parks in vector lanes.  hb_tap_mul says it with the instruction itself: 23 pairs stay in
 * scalar registers for the whole walk. */
constexpr int HBF_TAPS = 45;
struct HbChainTaps
{
  float2 p[(HBF_TAPS + 1) / 2]; // tap j = p[j / 2].x (j even) or .y
};

/* t[j] * x, both components (v_pk_mul_f32 is two IEEE multiplications, as the compiler's own) */
__device__ __forceinline__ float2 hb_tap_mul(const HbChainTaps& tp, int j, float2 x)
{
  float2 r;
  const float2 pr = tp.p[j / 2];
  if (j % 2 == 0)
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(r) : "v"(x), "s"(pr));
  else
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1]" : "=v"(r) : "v"(x), "s"(pr));
  return r;
}
/* (v.x o.x + -(0 o.y), v.x o.y + 0 o.x): the row's first component for both halves of the product, the entry out
 * of two scalar register pairs */
__device__ __forceinline__ float2 hb_osc_mul(float2 v, HbOsc o)
{
  float2 m, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(m) : "v"(v), "s"(o.xy));
  asm("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(m), "s"(o.z));
  return r;
}
__device__ __forceinline__ float2 hb_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }

/* RR consecutive outputs of one stage from its rows in registers: xe[u] = even row 2u of the group's window (row =
 * index into the stage's input with its L - 1 history rows in front: output k takes rows 2k .. 2k + L - 1), xc[r] =
 * the centre row 2r + HALF of output r; the stage's taps start at tap T of tp.  Order of the sum as in hb_group: tap
 * 0 twice, the even taps ascending, the centre tap last (DownConvert.cpp:526-543). */
template <int RR, int HALF, int T>
__device__ __forceinline__ void hb_rows(const float2* xe, const float2* xc, const HbChainTaps& tp, float2 (&acc)[RR])
{
  static_assert(HALF >= RR, "half-band group");
#pragma unroll
  for (int u = 0; u < RR + HALF; u++) // even row u: output r takes it with tap e[u - r]
  {
    const float2 x = xe[u];
#pragma unroll
    for (int r = 0; r < RR; r++)
    {
      const int j = u - r;
      if (j == 0)
      {
        acc[r] = hb_tap_mul(tp, T, x);
        acc[r] = hb_add(acc[r], hb_tap_mul(tp, T, x));
      }
      else if (j > 0 && j <= HALF)
        acc[r] = hb_add(acc[r], hb_tap_mul(tp, T + j, x));
    }
  }
#pragma unroll
  for (int r = 0; r < RR; r++)
    acc[r] = hb_add(acc[r], hb_tap_mul(tp, T + HALF + 1, xc[r]));
}

/* The rows of a group out of a ring whose slot row0 & 63 holds row 0 of the group's window.  One wave-uniform
 * decision per group and step: a window that does not reach the ring's end is one address and immediate offsets;
 * one that wraps masks each row's byte offset (an addition and a mask per read, no scalar work).  Both issue the
 * same reads in the same order. */
template <int RR, int HALF>
__device__ __forceinline__ void ring_rows(const float2 (*ring)[64], int row0, unsigned lane, float2 (&xe)[RR + HALF],
                                          float2 (&xc)[RR])
{
  constexpr int SPAN = 2 * (RR + HALF - 1) + 1;
  const int slot = row0 & (HBF_RING - 1);
  if (slot + SPAN <= HBF_RING)
  {
    const float2* p = &ring[slot][lane];
#pragma unroll
    for (int u = 0; u < RR + HALF; u++)
      xe[u] = p[2 * u * 64];
#pragma unroll
    for (int r = 0; r < RR; r++)
      xc[r] = p[(2 * r + HALF) * 64];
  }
  else
  {
    const char* base = reinterpret_cast<const char*>(&ring[0][0]);
    const unsigned a = (unsigned)slot * 512u + lane * 8u;
    auto at = [&](int row) { return *reinterpret_cast<const float2*>(base + ((a + (unsigned)row * 512u) & 0x7fffu)); };
#pragma unroll
    for (int u = 0; u < RR + HALF; u++)
      xe[u] = at(2 * u);
#pragma unroll
    for (int r = 0; r < RR; r++)
      xc[r] = at(2 * r + HALF);
  }
}

/* RR consecutive outputs into their ring slots (first output k0, nr of them valid) */
template <int RR>
__device__ __forceinline__ void ring_put(float2 (*ring)[64], int k0, int nr, unsigned lane, const float2 (&acc)[RR])
{
  const int slot = k0 & (HBF_RING - 1);
  if (nr == RR && slot <= HBF_RING - RR)
  {
    float2* p = &ring[slot][lane];
#pragma unroll
    for (int r = 0; r < RR; r++)
      p[r * 64] = acc[r];
  }
  else
  {
#pragma unroll
    for (int r = 0; r < RR; r++)
      if (r < nr)
        ring[(k0 + r) & (HBF_RING - 1)][lane] = acc[r];
  }
}

/* OSC: stage 0's input rows are not the mixed rows but (baseband, -) rows, and row r meets the RDS
 * oscillator's value osc[r] on its way into the sum -- (v osc.x - 0 osc.y, v osc.y + 0 osc.x) like
 * CRDSDownConvert::ProcessData writes it (DownConvert.cpp:464-465; the input's imaginary part is zero):
 * a - z is a + (-z), so with the table's two channel-independent products that is one multiplication and one
 * addition per component.
 *
 * Addresses.  Stage 0's fifteen rows of a wave and step are a wave-uniform 64-bit row pointer (one product per
 * step, the base of a buffer descriptor) plus fifteen 32-bit lane offsets that never change (lane + row * row
 * bytes: (2 (3 + H0) + 1) rows of CP float2 stay far below 4 GB).  No row is clamped and no load is conditional (a
 * group at the end of the input has fewer than four outputs, a step may have none for this wave; the compiler can
 * only wait for "all but the N youngest" loads, and it knows N -- the three younger sets that are still in flight
 * -- only if every path issues the same number): a group's window may reach up to HBF_SLACK rows past the last
 * input row, and the host keeps as many rows behind the input buffers and entries behind the oscillator's table.
 * What is read there only enters outputs that are not written. */
template <int H0, int H1, int H2, bool OSC = false>
__global__ __launch_bounds__(256) void k_halfband_chain(
    const float2* __restrict__ mix, const float2* __restrict__ hist1, const float2* __restrict__ hist2,
    float2* __restrict__ out, HbChainTaps tp, const HbStep* __restrict__ steps, const int* __restrict__ seg_first,
    unsigned C, unsigned CP, const HbOsc* __restrict__ osc, unsigned prio)
{
  wave_prio(prio);
  __shared__ float2 ring1[HBF_RING][64]; // stage 0's outputs, row i0 (>= -2 H1: history) at slot i0 & 63
  __shared__ float2 ring2[HBF_RING][64]; // stage 1's outputs
  constexpr int L1H = 2 * H1, L2H = 2 * H2; // history rows of stages 1 and 2
  static_assert(L1H + 34 <= HBF_RING && L2H + 18 <= HBF_RING, "ring size");
  static_assert((H0 + 2) + (H1 + 2) + (H2 + 2) <= HBF_TAPS, "tap table");
  static_assert(H0 % 2 == 1 && H1 % 2 == 1 && H2 % 2 == 1, "the centre rows are odd rows");
  constexpr int T1 = H0 + 2, T2 = T1 + H1 + 2; // the stages' first taps in tp
  const unsigned lane = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.y), w4 = 4 * w;
  const unsigned c0 = blockIdx.x * 64 + lane;
  // lanes past the batch's last channel do everything that channel's lane does, its stores included (the same
  // values to the same addresses): no lane mask anywhere
  const unsigned c = c0 < C ? c0 : C - 1;
  const int s_begin = seg_first[blockIdx.y], s_end = seg_first[blockIdx.y + 1];
  if (s_begin >= s_end)
    return;
  const size_t rowstride = CP; // (the history rows)
  // stage 0's input rows of this wave's group of a step: even rows 0, 2, .. 2 (3 + H0) and the four centres
  constexpr int NE = 4 + H0, NA = NE + 4;
  constexpr int NSET = HBF_NSET; // register sets: the rows of a step are fetched NSET - 1 steps ahead
  using Row = float2;
  Row xs[NSET][NA];
  const char* const gb = reinterpret_cast<const char*>(mix);
  const unsigned row_bytes = CP * (unsigned)sizeof(float2), lane_off = c * (unsigned)sizeof(float2);
  auto row_of = [](int i) { return i < NE ? 2 * i : 2 * (i - NE) + H0; };
  auto fetch_a = [&](Row (&x)[NA], int a_lo) {
    const char* rp = gb + (uint64_t)(unsigned)(2 * (a_lo + w4)) * row_bytes; // (32 x 32 -> 64 bits)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(rp), 0, -1, 0x00020000);
#pragma unroll
    for (int i = 0; i < NA; i++)
    {
      const unsigned off = lane_off + (unsigned)row_of(i) * row_bytes;
      const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0);
      x[i] = make_float2(__uint_as_float(v[0]), __uint_as_float(v[1]));
    }
  };
  // the rings' history (the first stretch of a call): rows -L1H .. -1 / -L2H .. -1
  {
    const HbStep f = steps[s_begin];
    if (2 * f.b_lo - L1H < 0)
      for (int i = w; i < L1H; i += 4)
        ring1[(i - L1H) & (HBF_RING - 1)][lane] = hist1[(size_t)i * rowstride + c];
    if (2 * f.c_lo - L2H < 0)
      for (int i = w; i < L2H; i += 4)
        ring2[(i - L2H) & (HBF_RING - 1)][lane] = hist2[(size_t)i * rowstride + c];
#pragma unroll
    for (int k = 0; k < NSET - 1; k++) // (a stretch's list has a multiple of NSET steps, empty ones at its end)
      fetch_a(xs[k], steps[s_begin + k].a_lo);
  }
  __syncthreads();
  // the step records travel a step ahead of their use too (a scalar load is a round trip to the L2 for a lone wave)
  const HbStep* __restrict__ sp = steps + s_begin;
  HbStep cur = sp[0];
  auto step = [&](int k, Row (&x)[NA], Row (&xn)[NA]) { // step sp[k] out of x; the rows of step sp[k + NSET - 1] into xn
    const HbStep st = cur;
    cur = sp[k + 1]; // (behind a stretch's last step: not a step, and not used)
    // the wave's place in the three groups of a step out of ONE register: the compiler would keep w, 2 w and 4 w
    int wq = w4;
    asm volatile("" : "+s"(wq));
    fetch_a(xn, st.a_lo + (int)((st.n >> HBF_FAR_SHIFT) & 63u));
    { // stage 0: four outputs per wave out of registers
      const int k0 = st.a_lo + wq;
      const int nr = min(4, st.a_lo + (int)(st.n & 31u) - k0);
      if (nr > 0)
      {
        float2 acc[4];
        if constexpr (!OSC)
          hb_rows<4, H0, 0>(x, x + NE, tp, acc);
        else
        {
          float2 xm[NA];
          const HbOsc* __restrict__ op = osc + 2 * k0; // wave-uniform entries: scalar loads at constant offsets
#pragma unroll
          for (int i = 0; i < NA; i++)
          {
          {
            xm[i] = hb_osc_mul(x[i], op[row_of(i)]);
            if (i % 4 == 3) // four entries (sixteen scalar registers) at a time: the taps need the rest
              __builtin_amdgcn_sched_barrier(0);
          }
          }
          hb_rows<4, H0, 0>(xm, xm + NE, tp, acc);
        }
        ring_put<4>(ring1, k0, nr, lane, acc);
        if (st.n & HBF_TAIL0) // the stage's last L1H outputs: the next call's history
        {
          const HbTails t = *reinterpret_cast<const HbTails*>(sp + k + (st.n >> HBF_TAILS_SHIFT));
#pragma unroll
          for (int r = 0; r < 4; r++)
            if (r < nr && k0 + r >= t.first1)
              hb_store_global(t.tail1 + ((size_t)(k0 + r - t.first1) * CP + c), acc[r]);
        }
      }
    }
    lds_barrier();
    { // stage 1: two outputs per wave out of ring 1 (row = output index of stage 0 + L1H)
      const int k0 = st.b_lo + (wq >> 1);
      const int nr = min(2, st.b_lo + (int)((st.n >> 5) & 15u) - k0);
      if (nr > 0)
      {
        float2 xe[2 + H1], xc[2], acc[2];
        ring_rows<2, H1>(ring1, 2 * k0 - L1H, lane, xe, xc);
        hb_rows<2, H1, T1>(xe, xc, tp, acc);
        ring_put<2>(ring2, k0, nr, lane, acc);
        if (st.n & HBF_TAIL1)
        {
          const HbTails t = *reinterpret_cast<const HbTails*>(sp + k + (st.n >> HBF_TAILS_SHIFT));
#pragma unroll
          for (int r = 0; r < 2; r++)
            if (r < nr && k0 + r >= t.first2)
              hb_store_global(t.tail2 + ((size_t)(k0 + r - t.first2) * CP + c), acc[r]);
        }
      }
    }
    lds_barrier();
    { // stage 2: one output per wave out of ring 2
      const int k0 = st.c_lo + (wq >> 2);
      if (k0 < st.c_lo + (int)((st.n >> 9) & 7u))
      {
        float2 xe[1 + H2], xc[1], acc[1];
        ring_rows<1, H2>(ring2, 2 * k0 - L2H, lane, xe, xc);
        hb_rows<1, H2, T2>(xe, xc, tp, acc);
        { // (a store by descriptor like the loads: the row's address is scalar work, the lane's part never changes)
          char* op = reinterpret_cast<char*>(out) + (uint64_t)(unsigned)k0 * row_bytes;
          typedef unsigned hb_u2 __attribute__((ext_vector_type(2)));
          hb_u2 v;
          v[0] = __float_as_uint(acc[0].x);
          v[1] = __float_as_uint(acc[0].y);
          __builtin_amdgcn_raw_buffer_store_b64(v, __builtin_amdgcn_make_buffer_rsrc(op, 0, -1, 0x00020000), lane_off, 0, 0);
        }
      }
    }
    return (st.n & HBF_LAST) != 0u;
  };
  for (bool last = false; !last; sp += NSET)
  {
#pragma unroll
    for (int k = 0; k < NSET; k++)
      last = step(k, xs[k], xs[(k + NSET - 1) % NSET]);
  }
}

/* Workgroup = 64 channels x RF_TI outputs.  The T-1+RF_TI input rows of the tile are staged once
 * in LDS ([row][channel]: conflict-free reads), because every input row is needed by T different
 * outputs and re-reading it from L2 for each made the kernel L2-bandwidth bound.
 * E = float2 for the complex / two-stream filters, float for the RDS matched filter. */
/* Per-channel ring origins (fmd_batch_reset_channels): a channel reset when the batch's
 * ring phase was origin[c] is origin[c] samples behind the batch, so its output i has phase
 * (g0 + i - origin[c]) mod T.  ring_wave_g0 gives every lane its own start phase (*lane_g0) and returns the
 * wave's common one where all of its channels share one origin (the usual case: nothing reset, a capture's
 * channels or all of them reset together), -1 where they differ.  Lanes past C take lane 0's origin, so that
 * they never split a wave.  Call it with every lane of the wave active. */
__device__ __forceinline__ int ring_wave_g0(const unsigned* __restrict__ origin, unsigned c, unsigned C, unsigned g0,
                                            int T, unsigned* lane_g0)
{
  const unsigned o_lane = c < C ? origin[c] : 0u;
  const unsigned o0 = (unsigned)__builtin_amdgcn_readfirstlane((int)o_lane); // lane 0: a channel of the batch
  const unsigned o = c < C ? o_lane : o0;
  *lane_g0 = (g0 + (unsigned)T - o) % (unsigned)T;
  if (__ballot(o != o0) != 0ull)
    return -1;
  return (int)((g0 + (unsigned)T - o0) % (unsigned)T);
}

/* Output i of one lane with a phase of its own (a wave of mixed origins): the T ages a0, ..., T-1, 0, ..., a0-1 in
 * one loop of T trips for every lane, the age and the row pointer wrapping per lane.  `now` points at the input of
 * age 0, age a sits `a * stride` elements before it.  The same products and sums in the same order as the uniform
 * forms (whose sums start from -0: -0 + k x is k x). */
template <typename E>
__device__ __forceinline__ E ring_one_mixed(const E* __restrict__ now, size_t stride, unsigned a0, int T,
                                            const float* __restrict__ taps)
{
  const E* __restrict__ p = now - a0 * stride;
  E acc = rf_mul(taps[a0], *p);
  unsigned a = a0;
  for (int s = 1; s < T; s++)
  {
    const bool wrap = a + 1 == (unsigned)T;
    a = wrap ? 0u : a + 1;
    p = wrap ? now : p - stride;
    rf_acc(acc, taps[a], *p);
  }
  return acc;
}

template <typename E, bool ORG>
__device__ __forceinline__ void ring_fir_tile(E* __restrict__ rtile, const E* __restrict__ in, E* __restrict__ out,
                                              unsigned n, int T, const float* __restrict__ taps, unsigned g0,
                                              unsigned C, unsigned CP, unsigned Hout,
                                              const unsigned* __restrict__ origin)
{
  const unsigned lane = threadIdx.x;
  const unsigned y = (unsigned)__builtin_amdgcn_readfirstlane((int)threadIdx.y); // 0..3, wave-uniform
  const unsigned c0 = blockIdx.x * 64 + lane;
  const unsigned c = c0 < C ? c0 : C - 1;
  const unsigned i0 = blockIdx.y * RF_TI;
  const unsigned nt = min((unsigned)RF_TI, n - i0);
  const unsigned rows = (unsigned)T - 1 + nt;
  // buffer row of x[i - a] is (T-1 + i - a); the tile starts at buffer row i0
  for (unsigned r = y; r < rows; r += 4)
    rtile[r * 64 + lane] = in[(size_t)(i0 + r) * CP + c];
  __syncthreads();
  unsigned lane_g0 = g0;
  if constexpr (ORG)
  { // (the four waves of a workgroup hold the same 64 channels: the same answer in all of them)
    const int wg0 = ring_wave_g0(origin, c0, C, g0, T, &lane_g0);
    if (wg0 < 0)
    {
      if (c0 >= C)
        return;
      for (unsigned q = y; q < nt; q += 4)
      {
        const unsigned i = i0 + q;
        const E* base = rtile + (size_t)((unsigned)T - 1 + q) * 64 + lane;
        out[(size_t)(Hout + i) * CP + c] = ring_one_mixed<E>(base, 64, (lane_g0 + i) % (unsigned)T, T, taps);
      }
      return;
    }
    g0 = (unsigned)wg0;
  }
  if (c0 >= C)
    return;
  for (unsigned q = y; q < nt; q += 4)
  {
    const unsigned i = i0 + q;
    const int a0 = (int)((g0 + i) % (unsigned)T);
    // newest sample (age 0) sits at tile row T-1+q; age a at row T-1+q-a
    const E* base = rtile + (size_t)((unsigned)T - 1 + q) * 64 + lane;
    E acc = rf_mul(taps[a0], base[-(ptrdiff_t)a0 * 64]);
#pragma unroll 4
    for (int a = a0 + 1; a < T; a++) // ages a0+1 .. T-1
      rf_acc(acc, taps[a], base[-(ptrdiff_t)a * 64]);
#pragma unroll 4
    for (int a = 0; a < a0; a++) // then the ring wraps: ages 0 .. a0-1
      rf_acc(acc, taps[a], base[-(ptrdiff_t)a * 64]);
    out[(size_t)(Hout + i) * CP + c] = acc;
  }
}

template <typename E>
__global__ __launch_bounds__(256) void k_ring_fir(const E* __restrict__ in, E* __restrict__ out,
                                                  unsigned n, int T, const float* __restrict__ taps,
                                                  unsigned g0, unsigned C, unsigned CP, unsigned Hout)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char rtile_raw[];
  ring_fir_tile<E, false>(reinterpret_cast<E*>(rtile_raw), in, out, n, T, taps, g0, C, CP, Hout, nullptr);
}

/* k_ring_fir for a batch with reset channels: per-channel ring origins (RDS low-pass, matched filter) */
template <typename E>
__global__ __launch_bounds__(256) void k_ring_fir_org(const E* __restrict__ in, E* __restrict__ out,
                                                      unsigned n, int T, const float* __restrict__ taps,
                                                      unsigned g0, unsigned C, unsigned CP, unsigned Hout,
                                                      const unsigned* __restrict__ origin)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char rtile_raw[];
  ring_fir_tile<E, true>(reinterpret_cast<E*>(rtile_raw), in, out, n, T, taps, g0, C, CP, Hout, origin);
}

/* The same filter for the two float2 instances on the heavy part of the post chain (RDS low-pass,
 * audio low-pass), without LDS and without a barrier: thread = (channel lane, RG consecutive
 * outputs), rows straight from L2 / L1.  Output i sums times B, B-1, ..., i-T+1 and then i, i-1,
 * ..., B+1 with B = i - ((g0 + i) mod T), the time of the sample in ring slot 0; consecutive
 * outputs of one ring period share B, so a group walks the rows all of its outputs take once
 * (four taps per row, contiguous in the table: age = output - row), and the few rows only some of
 * them take on their own.  Every output's accumulator starts at -0 (x + -0 = x for every x), the
 * order is the reference's.  A group that straddles a ring period is done as two groups. */
#ifndef FMD_RG
#define FMD_RG 8 // (4 until round 5: 8 outputs per thread read 4.5 rows per output instead of 8 -- 0.061 against 0.092 ms alone for the RDS low-pass, +1.7 % whole path; 12 and 16: no better)
#endif
constexpr int RG = FMD_RG;
#ifndef FMD_RING_UNROLL
#define FMD_RING_UNROLL 8 // rows in flight per thread in ring_group's two long loops
#endif

__device__ __forceinline__ float rf_neg_zero(float*) { return -0.0f; }
__device__ __forceinline__ float2 rf_neg_zero(float2*) { return make_float2(-0.0f, -0.0f); }

template <int RR, typename E>
__device__ __forceinline__ void ring_group(const E* __restrict__ in, E* __restrict__ out,
                                           unsigned i, int T, const float* __restrict__ taps,
                                           unsigned g0, unsigned c, unsigned CP, unsigned Hout, bool store)
{
  const int a0 = (int)((g0 + i) % (unsigned)T); // a0 + RR - 1 <= T - 1: one ring period
  E acc[RR];
#pragma unroll
  for (int r = 0; r < RR; r++)
    acc[r] = rf_neg_zero((E*)nullptr);
  // buffer row of time t is T - 1 + t
  const E* __restrict__ p1 = in + (size_t)((unsigned)T - 1 + i - (unsigned)a0) * CP + c; // time B
  const float* __restrict__ k1 = taps + a0;
  const int n1 = T - a0 - (RR - 1); // rows B .. i+RR-T, taken by every output: ages a0 + r + s
#pragma unroll FMD_RING_UNROLL
  for (int s = 0; s < n1; s++)
  {
    const E x = *p1;
    p1 -= CP;
#pragma unroll
    for (int r = 0; r < RR; r++)
      rf_acc(acc[r], k1[s + r], x);
  }
#pragma unroll
  for (int m = 0; m < RR - 1; m++) // the oldest rows: output r takes RR-1-r of them, up to age T-1
  {
    const E x = *p1;
    p1 -= CP;
#pragma unroll
    for (int r = 0; r < RR - 1 - m; r++)
      rf_acc(acc[r], taps[T - (RR - 1) + r + m], x);
  }
  const E* __restrict__ p2 = in + (size_t)((unsigned)T - 1 + i + RR - 1) * CP + c; // time i+RR-1
#pragma unroll
  for (int m = 0; m < RR - 1; m++) // the newest rows: output r takes the last r of them, from age 0
  {
    const E x = *p2;
    p2 -= CP;
#pragma unroll
    for (int r = RR - 1 - m; r < RR; r++)
      rf_acc(acc[r], taps[r - (RR - 1 - m)], x);
  }
#pragma unroll FMD_RING_UNROLL
  for (int s = 0; s < a0; s++) // rows i .. B+1, taken by every output: ages r + s
  {
    const E x = *p2;
    p2 -= CP;
#pragma unroll
    for (int r = 0; r < RR; r++)
      rf_acc(acc[r], taps[s + r], x);
  }
  if (store)
  {
#pragma unroll
    for (int r = 0; r < RR; r++)
      out[(size_t)(Hout + i + r) * CP + c] = acc[r];
  }
}

template <int RR, typename E>
__device__ __forceinline__ void ring_dispatch(unsigned take, const E* __restrict__ in,
                                              E* __restrict__ out, unsigned i, int T,
                                              const float* __restrict__ taps, unsigned g0, unsigned c,
                                              unsigned CP, unsigned Hout, bool store)
{ // take is wave-uniform: one scalar branch per size
  if (take == (unsigned)RR)
    ring_group<RR, E>(in, out, i, T, taps, g0, c, CP, Hout, store);
  else if constexpr (RR > 1)
    ring_dispatch<RR - 1, E>(take, in, out, i, T, taps, g0, c, CP, Hout, store);
}

template <typename E>
__global__ __launch_bounds__(256) void k_ring_fir4(const E* __restrict__ in, E* __restrict__ out,
                                                   unsigned n, int T, const float* __restrict__ taps,
                                                   unsigned g0, unsigned C, unsigned CP, unsigned Hout,
                                                   unsigned prio)
{
  // the real instance is the matched filter between two lane-per-channel kernels of the light part:
  // short, and the light part should be over before the next FIR starts -> issue first, like them (prio 3)
  wave_prio(prio);
  const unsigned c = blockIdx.x * 64 + threadIdx.x; // < CP: the row buffers are padded
  const unsigned y = (unsigned)__builtin_amdgcn_readfirstlane((int)threadIdx.y);
  unsigned i = (blockIdx.y * blockDim.y + y) * RG;
  if (i >= n)
    return;
  const bool store = c < C;
  unsigned left = min((unsigned)RG, n - i);
  while (left)
  { // as many outputs as stay within one ring period
    const unsigned room = (unsigned)T - (g0 + i) % (unsigned)T;
    const unsigned take = min(left, room);
    ring_dispatch<RG, E>(take, in, out, i, T, taps, g0, c, CP, Hout, store);
    i += take;
    left -= take;
  }
}

/* k_ring_fir4 for a batch with reset channels: per-channel ring origins (RDS low-pass, matched filter).  A wave
 * whose channels share one origin runs the groups above with its own g0 (take stays wave-uniform); a mixed wave
 * takes its outputs one by one, each lane in its own phase (ring_one_mixed). */
template <typename E>
__global__ __launch_bounds__(256) void k_ring_fir4_org(const E* __restrict__ in, E* __restrict__ out,
                                                       unsigned n, int T, const float* __restrict__ taps,
                                                       unsigned g0, unsigned C, unsigned CP, unsigned Hout,
                                                       unsigned prio, const unsigned* __restrict__ origin)
{
  wave_prio(prio);
  const unsigned c = blockIdx.x * 64 + threadIdx.x; // < CP: the row buffers are padded
  const unsigned y = (unsigned)__builtin_amdgcn_readfirstlane((int)threadIdx.y);
  unsigned i = (blockIdx.y * blockDim.y + y) * RG;
  if (i >= n)
    return;
  const bool store = c < C;
  unsigned left = min((unsigned)RG, n - i);
  unsigned lane_g0 = g0;
  const int wg0 = ring_wave_g0(origin, c, C, g0, T, &lane_g0);
  if (wg0 < 0)
  {
    for (; left; i++, left--)
    {
      const unsigned a0 = (lane_g0 + i) % (unsigned)T;
      const E* __restrict__ now = in + (size_t)((unsigned)T - 1 + i) * CP + c; // age 0
      const E acc = ring_one_mixed<E>(now, CP, a0, T, taps);
      if (store)
        out[(size_t)(Hout + i) * CP + c] = acc;
    }
    return;
  }
  g0 = (unsigned)wg0;
  while (left)
  {
    const unsigned room = (unsigned)T - (g0 + i) % (unsigned)T;
    const unsigned take = min(left, room);
    ring_dispatch<RG, E>(take, in, out, i, T, taps, g0, c, CP, Hout, store);
    i += take;
    left -= take;
  }
}

/* ------------------------------------------------------------------------------------------ */
/* K5: RDS recurrences at the RDS rate.  The matched filter between the two serial kernels     */
/*     (cFirFilter::Process(real), FirFilter.cpp:360-377) runs time-parallel in k_ring_fir.      */
/* ------------------------------------------------------------------------------------------ */
/* OBS (the observing forms of the bit recovery): *pre takes the syndrome before the error correction, *flips the
 * bits the Meggitt loop flipped (the reference's correctedbits, RDSProcess.cpp:398-410: counted and never used). */
template <bool OBS = false>
__device__ __forceinline__ uint32_t rds_check_block(uint32_t& in_bits, uint32_t offset, bool fec,
                                                    uint32_t* pre = nullptr, unsigned* flips = nullptr)
{
  const uint32_t parckh[16] = {0x2DC, 0x16E, 0x0B7, 0x287, 0x39F, 0x313, 0x355, 0x376,
                               0x1BB, 0x201, 0x3DC, 0x1EE, 0x0F7, 0x2A7, 0x38F, 0x31B};
  uint32_t tb = 0x3FFFFFF & in_bits;
  uint32_t syn = tb >> 16;
#pragma unroll
  for (int i = 0; i < 16; i++)
  {
    if (tb & 0x8000)
      syn ^= parckh[i];
    tb <<= 1;
  }
  syn ^= offset;
  if constexpr (OBS)
    *pre = syn;
  if (syn && fec)
  {
    uint32_t mask = 1u << 25;
    for (int i = 0; i < 16; i++)
    {
      if (syn & 0x200)
      {
        if ((syn & 0x1F) == 0)
        {
          in_bits ^= mask;
          syn <<= 1;
          if constexpr (OBS)
            (*flips)++;
        }
        else
        {
          syn <<= 1;
          syn ^= 0x5B9;
        }
      }
      else
        syn <<= 1;
      mask >>= 1;
    }
    syn &= 0x3FF;
  }
  return syn;
}

/* K5a: ProcessRdsPll (RDSProcess.cpp:222-270), one lane per channel.  Output = de-rotated
 *      imaginary part, written behind the T_mf-1 history rows the matched filter needs.
 *      Four waves (one per SIMD) share the 16 KB sine / cosine table of a workgroup: a quarter as many
 *      CUs carry one during the 0.2-0.5 ms the kernel runs, which matters to the whole-CU resampler. */
#ifndef FMD_RP_WAVES
#define FMD_RP_WAVES 4
#endif
constexpr int RP_WAVES = FMD_RP_WAVES; // channel groups (waves) of a workgroup that share one sine table in LDS
__global__ __launch_bounds__(64 * RP_WAVES) void k_rds_pll(const float2* __restrict__ lpf, unsigned R, unsigned C,
                                                unsigned CP, RdsConsts k, ChannelState st,
                                                float* __restrict__ rpll, unsigned Hout,
                                                const double* __restrict__ sctab_g, FmdSincosTab sct)
{
  __shared__ double sctab[2 * FMD_SINCOS_TAB_SIZE];
  __builtin_amdgcn_s_setprio(3);
  for (unsigned i = threadIdx.y * 64 + threadIdx.x; i < 2 * FMD_SINCOS_TAB_SIZE; i += 64 * RP_WAVES)
    sctab[i] = sctab_g[i];
  __syncthreads();
  const unsigned c = (blockIdx.x * RP_WAVES + threadIdx.y) * 64 + threadIdx.x;
  if (c >= C)
    return;
  float phase = st.F(F_R_PHASE)[c], freq = st.F(F_R_FREQ)[c];
  float* __restrict__ o = rpll + (size_t)Hout * CP + c;
  /* The input travels a whole tile ahead of its use: the loads of tile n + 1 are in flight while
   * tile n goes through the recurrence (one load per sample, issued one sample ahead, had to come
   * back within an iteration -- 0.2 us; beside the bandwidth kernels a load takes several times that
   * and the kernel took 0.56 ms inside the pipeline against 0.23 ms alone). */
  constexpr unsigned PT = 16;
  float2 nxt[PT];
#pragma unroll
  for (unsigned u = 0; u < PT; u++)
    nxt[u] = lpf[(size_t)min(u, R - 1) * CP + c];
  for (unsigned i0 = 0; i0 < R; i0 += PT)
  {
    float2 cur[PT];
#pragma unroll
    for (unsigned u = 0; u < PT; u++)
      cur[u] = nxt[u];
#pragma unroll
    for (unsigned u = 0; u < PT; u++) // clamped: past the end the last row again (never used)
      nxt[u] = lpf[(size_t)min(i0 + PT + u, R - 1) * CP + c];
    const unsigned cnt = min(PT, R - i0);
#pragma unroll
    for (unsigned u = 0; u < PT; u++)
    {
      if (u < cnt)
      {
        const float2 in = cur[u];
        float sn, cs;
        fmd_sincos_tab(phase, sctab, sct, &sn, &cs);
        const float tr = cs * in.x - sn * in.y;
        const float ti = cs * in.y + sn * in.x;
        const float err = -fmd_rds_arctan2(ti, tr);
        freq += (k.pll_beta * err);
        freq = (freq > k.nco_hl) ? k.nco_hl : ((freq < k.nco_ll) ? k.nco_ll : freq);
        phase += (freq + k.pll_alpha * err);
        *o = ti;
        o += CP;
      }
    }
  }
  st.F(F_R_PHASE)[c] = fmodf(phase, (float)FMD_K_2PI); // RDSProcess.cpp:269
  st.F(F_R_FREQ)[c] = freq;
}

/* K5b: after the matched filter (k_ring_fir<float>): squaring + bit-sync resonator
 *      (RDSProcess.cpp:137-142, IirFilter.cpp:78-87), peak slicer (:144-179), ProcessNewRdsBit
 *      (:272-375) and CheckBlock with Meggitt FEC (:377-431).  One lane per channel.  Sliced
 *      bits are queued per lane and the block-sync state machine drains the queue once per
 *      RB_TILE samples, so the wave does not run it on every sample just because some lane has
 *      a bit. */
constexpr int RB_TILE = 32;

/* What the observing forms of the bit recovery (k_rds_bits_obs; fmd_batch_set_rds_blocks)
 * take beside k_rds_bits' arguments.  The counters are the observation's and not the decoder's: an array of their
 * own, [RQ_N][CP] in coalesced rows, that no reset, retune, import or load touches.  A block record is 32 bytes on
 * the device, two 16-byte stores: the 24 bytes of fmd_rds_block and 8 of padding. */
enum RdsQuality
{
  RQ_BITS,
  RQ_CANDIDATES,
  RQ_BLOCKS,
  RQ_CORRECTED,
  RQ_FAILED,
  RQ_ACQUIRED,
  RQ_LOST,
  RQ_GROUPS,
  RQ_N
};
struct RdsObs
{
  unsigned* quality = nullptr;     // [RQ_N][CP]
  uint4* blocks = nullptr;         // the call's block queue, two uint4 per record
  unsigned* block_count = nullptr; // records appended so far (counts on past block_cap: the host works out the loss)
  unsigned block_cap = 0;
};

/* The bit recovery proper, and its two observing forms: ONE text (fmd_rds_bits.inc), like the audio tail's.  A call
 * submitted with the block observation off launches k_rds_bits, which is what it always was. */
__global__ __launch_bounds__(256) void k_rds_bits(const float* __restrict__ mf, unsigned R, unsigned C,
                                                 unsigned CP, RdsConsts k, ChannelState st,
                                                 uint32_t call_index, RdsGroupRec* __restrict__ queue,
                                                 unsigned* __restrict__ queue_count, unsigned queue_cap,
                                                 float* __restrict__ tap_sync, int write_taps)
{
  constexpr int OBS = 0;
  const RdsObs ob{};
#include "fmd_rds_bits.inc"
}

/* The bit recovery of a call submitted with the block observation on (fmd_batch_set_rds_blocks): the same decoder,
 * bit for bit, plus the channel's reception counters (RECORD false: FMD_RDS_BLOCKS_COUNT) and a record of every
 * block decision in the call's block queue (RECORD true: FMD_RDS_BLOCKS_RECORD). */
template <bool RECORD>
__global__ __launch_bounds__(256) void k_rds_bits_obs(const float* __restrict__ mf, unsigned R, unsigned C,
                                                     unsigned CP, RdsConsts k, ChannelState st,
                                                     uint32_t call_index, RdsGroupRec* __restrict__ queue,
                                                     unsigned* __restrict__ queue_count, unsigned queue_cap,
                                                     float* __restrict__ tap_sync, int write_taps, RdsObs ob)
{
  constexpr int OBS = RECORD ? 2 : 1;
#include "fmd_rds_bits.inc"
}

} // namespace fmd
