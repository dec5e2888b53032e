/*
 * fmd_k_mpx.hip.h -- the demodulated multiplex (MPX) as an output: k_mpx_out transposes the serial stage's
 * time-major baseband rows into one contiguous row per channel, as float or as 16-bit integers (FMD_MPX_*);
 * k_debug_mpx is the device build of the conversion for fmd_debug_math.
 * Part of fmd_kernels.hip.h (layout, numerics contract and citations: see there and fmd_k_common.hip.h).
 */
#pragma once

#include "fmd_k_common.hip.h"

namespace fmd
{

/* The store policies of k_mpx_out: the call's `mpx_format`.  A lane ends with PER consecutive samples of one
 * channel, 16 bytes either way. */
struct MpxF32
{ // the float the FM PLL left (FmDecode.cpp:433), as is
  using elem_t = float;
  static constexpr unsigned PER = 4;
};
struct MpxS16
{ // fmd_f32_to_mpx16 of it, host byte order
  using elem_t = int16_t;
  static constexpr unsigned PER = 8;
};

constexpr unsigned MPX_T = 64; // time steps of a tile: 256 contiguous bytes of a float row, 128 of an int16 row

/* k_mpx_out (its body is fmd_mpx_tile.inc, one text with the selected writer below):
 * One workgroup (4 waves) per tile of 64 channels x MPX_T time steps of `in`, the `.x` halves of the float2 rows
 * [t][CP] the serial stage wrote (in = first data row, as floats); out: row c at out + c * stride elements.
 *
 * Reads: wave w takes the tile's rows 16 jj + 4 w + e (jj, e = 0..3), a lane one channel: per row the 64 lanes
 * read the `.x` of 64 consecutive float2 (512 contiguous bytes; rows at or behind M are not read).
 *
 * LDS image (16 KiB): channel-major, a channel's 64 floats are one 256-byte bank row of sixteen 16-byte slots;
 * slot j (time steps 4 j .. 4 j + 3) of channel c lies at slot (j + (c >> 1)) % 16 of row c.
 *   writes  ds_write_b128, one slot a lane (four rows of one channel): bank = (a / 4) % 32, eight consecutive
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
 * reaches over M, is stored element by element, never at or behind M. */
template <class Fmt>
__global__ __launch_bounds__(256) void k_mpx_out(const float* __restrict__ in, unsigned M, unsigned C, unsigned CP,
                                                 typename Fmt::elem_t* __restrict__ out, size_t stride)
{
#define FMD_MPX_SRC(c) (row0 + (c))
#define FMD_MPX_SKIPPED(c) (row0 + (c) >= C)
#define FMD_MPX_DST(c) (row0 + (c))
#include "fmd_mpx_tile.inc"
#undef FMD_MPX_SRC
#undef FMD_MPX_SKIPPED
#undef FMD_MPX_DST
}

/* The selected writer (fmd_batch_select_mpx): tiles of 64 list entries x MPX_T time steps, grid ((n + 63) / 64, tiles
 * of time).  ent[e] = (channel the entry reads, output row it writes), e < n, sorted by channel by the host: the LDS
 * image, its conflict-free reads and writes and the 16-byte stores are k_mpx_out's (the layout argument above is about
 * tile rows, whatever channels they hold); the loads are per-lane gathers of the 8-byte float2 of the entry's channel
 * out of the [t][CP] rows -- neighbouring channels of the sorted list share a 64- or 128-byte request, a lone
 * channel takes one 32-byte sector per time step for its 4 bytes.  Output rows >= n and samples at or behind M are
 * never written. */
template <class Fmt>
__global__ __launch_bounds__(256) void k_mpx_out_sel(const float* __restrict__ in, unsigned M, unsigned n, unsigned CP,
                                                     const int2* __restrict__ ent,
                                                     typename Fmt::elem_t* __restrict__ out, size_t stride)
{
  // (entries at or behind n: the last one's channel is read again, none is stored)
#define FMD_MPX_SRC(c) ((unsigned)ent[min(row0 + (c), n - 1u)].x)
#define FMD_MPX_SKIPPED(c) (row0 + (c) >= n)
#define FMD_MPX_DST(c) ((unsigned)ent[row0 + (c)].y)
#include "fmd_mpx_tile.inc"
#undef FMD_MPX_SRC
#undef FMD_MPX_SKIPPED
#undef FMD_MPX_DST
}

/* The device build of fmd_f32_to_mpx16 on an array (fmd_debug_math, what = 9): the result as a float. */
__global__ __launch_bounds__(64) void k_debug_mpx(unsigned n, const float* __restrict__ a, float* __restrict__ o0,
                                                  float* __restrict__ o1)
{
  for (unsigned i = blockIdx.x * 64 + threadIdx.x; i < n; i += gridDim.x * 64)
  {
    o0[i] = (float)fmd_f32_to_mpx16(a[i]);
    o1[i] = 0.0f;
  }
}

} // namespace fmd
