/*
 * fmd_k_feed.hip.h -- the mono feed at sample_rate_pcm / 2 or / 3 beside the audio (FMD_FEED_*): k_feed_out runs the
 * decimating low-pass over the time-major rows x[g] = (L[g] + R[g]) * 0.5f the feed forms of the audio tail left in
 * the batch's scratch, and writes one contiguous row per channel, as float or as 16-bit integers.
 * Part of fmd_kernels.hip.h (layout, numerics contract and citations: see there and fmd_k_common.hip.h).
 */
#pragma once

#include "fmd_k_common.hip.h"

namespace fmd
{

/* The store policies of k_feed_out: the call's `feed_format`.  A lane ends with PER consecutive samples of one
 * channel, 16 bytes either way. */
struct FeedF32
{ // the filter's float sum, as is
  using elem_t = float;
  static constexpr unsigned PER = 4;
};
struct FeedS16
{ // fmd_f32_to_s16 of it (the audio's rule), host byte order
  using elem_t = int16_t;
  static constexpr unsigned PER = 8;
};

constexpr unsigned FEED_T = 64;        // outputs of a tile: 256 contiguous bytes of a float row, 128 of an int16 row
constexpr unsigned FEED_TAPS_MAX = 75; // make_kaiser_lp's cap (fmd_design.hpp); the two divisors take 49 and 73

/* k_feed_out (its body is fmd_feed_tile.inc, one text with the selected writer below):
 * One workgroup (4 waves) per tile of 64 channels x FEED_T outputs.  x = the scratch [H + Amax][CP], H = T - 1 rows of
 * history in front of the call's A rows; output j of the call (j < n) is
 *   y = sum over k = 0 .. T - 1 of taps[k] * x[(H + p0 + j D - k) * CP + c],
 * p0 = the call's first frame that is a multiple of D in the feed's own count of frames (0 <= p0 < D): the host's
 * to know.  The sum starts at 0 and takes the taps in ascending order, multiply and add rounded separately
 * (__fmul_rn / __fadd_rn: never contracted), so a numpy float32 loop over k gives the same bits.
 *
 * Reads: wave w takes the tile's outputs 16 jj + 4 w + e (jj, e = 0..3), a lane one channel: per tap and output the
 * 64 lanes read 64 consecutive floats of one scratch row (256 contiguous bytes).  The four outputs of a step walk
 * four rows D apart down the taps: every row is read T / D times by the tile, out of the L1 / L2 behind the first.
 * The taps are wave-uniform: staged in LDS once, every lane of a wave reads the same word (a broadcast, no conflict).
 * Outputs at or behind n are not computed from rows of their own (the call's last output's rows are read instead:
 * nothing behind row H + A - 1 is touched).
 *
 * LDS image (16 KiB + the taps): k_mpx_out's (fmd_k_mpx.hip.h) with outputs where that one has time steps --
 * channel-major, a channel's 64 floats are one 256-byte bank row of sixteen 16-byte slots; slot j (outputs 4 j ..
 * 4 j + 3) of channel c lies at slot (j + (c >> 1)) % 16 of row c.
 *   writes  ds_write_b128, one slot a lane (four outputs of one channel): bank = (a / 4) % 32, eight consecutive
 *           lanes a cycle.  Lane l holds channel (l & 48) + 2 (l & 7) + ((l >> 3) & 1): the eight lanes of a cycle
 *           hold every second channel, c >> 1 = 8 a + k for k = 0..7, slots (j + k) % 8 -- eight different
 *           slots of the 32 banks: 0 conflicts.
 *   reads   ds_read_b128, bank = (a / 4) % 64, sixteen lanes a cycle ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the
 *           same + 32).  F32: lane l reads slot l & 15 of channel c0 + (l >> 4), c0 a multiple of 4 -- a cycle holds
 *           slots {0-3,12-15} of one channel and {4-11} of its pair (or the other way round): same c >> 1, so the
 *           sixteen slots are the sixteen of a bank row, rotated: 0 conflicts.  S16: lane l reads slots 2 (l & 7)
 *           and 2 (l & 7) + 1 of channel c0 + (l >> 3), c0 a multiple of 8 -- a cycle holds the even (odd) slots
 *           of a pair's two half rows and of the next pair's, rotated by one more: sixteen different slots, 0
 *           conflicts.
 * Stores: 16 bytes a lane; sixteen (F32) / eight (S16) consecutive lanes fill 256 / 128 contiguous bytes of a channel's
 * row.  Rows start on 16-byte boundaries (pointer and stride are the entry point's to check) and a tile starts at a
 * multiple of 64 elements, so every group is aligned.  Channels >= C are not stored; the call's last tile, where it
 * reaches over n, is stored element by element, never at or behind n.  No scratch memory (private segment 0). */
template <class Fmt>
__global__ __launch_bounds__(256) void k_feed_out(const float* __restrict__ x, const float* __restrict__ taps,
                                                  unsigned T, unsigned D, unsigned p0, unsigned n, unsigned C,
                                                  unsigned CP, typename Fmt::elem_t* __restrict__ out, size_t stride)
{
#define FMD_FEED_SRC(c) (row0 + (c))
#define FMD_FEED_SKIPPED(c) (row0 + (c) >= C)
#define FMD_FEED_DST(c) (row0 + (c))
#include "fmd_feed_tile.inc"
#undef FMD_FEED_SRC
#undef FMD_FEED_SKIPPED
#undef FMD_FEED_DST
}

/* The selected writer (fmd_batch_select_feed): tiles of 64 list entries x FEED_T outputs, grid ((ns + 63) / 64, tiles
 * of outputs).  ent[e] = (channel the entry reads, output row it writes), e < ns, sorted by channel by the host: the
 * LDS image, its conflict-free reads and writes and the 16-byte stores are k_feed_out's (the layout argument above is
 * about tile rows, whatever channels they hold); the loads are per-lane gathers of the entry's channel out of the
 * scratch rows -- neighbouring channels of the sorted list share a request.  Output rows >= ns and samples at or
 * behind n are never written. */
template <class Fmt>
__global__ __launch_bounds__(256) void k_feed_out_sel(const float* __restrict__ x, const float* __restrict__ taps,
                                                      unsigned T, unsigned D, unsigned p0, unsigned n, unsigned ns,
                                                      unsigned CP, const int2* __restrict__ ent,
                                                      typename Fmt::elem_t* __restrict__ out, size_t stride)
{
  // (entries at or behind ns: the last one's channel is read again, none is stored)
#define FMD_FEED_SRC(c) ((unsigned)ent[min(row0 + (c), ns - 1u)].x)
#define FMD_FEED_SKIPPED(c) (row0 + (c) >= ns)
#define FMD_FEED_DST(c) ((unsigned)ent[row0 + (c)].y)
#include "fmd_feed_tile.inc"
#undef FMD_FEED_SRC
#undef FMD_FEED_SKIPPED
#undef FMD_FEED_DST
}

} // namespace fmd
