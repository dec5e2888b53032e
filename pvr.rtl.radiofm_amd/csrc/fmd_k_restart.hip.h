/*
 * fmd_k_restart.hip.h -- k_channel_restart: restarts single channels of a running batch at a call
 * boundary (fmd_batch_retune_channels); k_channel_reset (below) resets them (fmd_batch_reset_channels).
 * A retuned channel takes over the carried state of the batch's silent twin (a one-channel batch of
 * the same geometry fed zeros, csrc/fmd_batch.hip) and a new cFineTuner table row; every other channel
 * is left alone.
 *
 * What is copied is a list of regions (RestartRegion, built once by the host: the table is in
 * fmd_batch.hip, restart_regions).  A region is one buffer of per-channel state, `rows` elements per
 * channel of 2, 4 or 8 bytes, element (row, c) at base + row * row_stride + c * ch_stride (in elements):
 * time-major history rows have row_stride = CP and ch_stride = 1, the IF history (channel-major) the
 * other way round.  The source is channel 0 of the twin's buffer.
 *
 * The edited channels come sorted: consecutive threads take consecutive edits of one (region, row,
 * element), so with many edits the writes of a wavefront land in neighbouring channels of one row
 * (coalesced) and the twin's element is one broadcast read.
 */
#pragma once

#include "fmd_k_common.hip.h"

namespace fmd
{

constexpr int kRestartMaxRegions = 24;

struct RestartRegion
{
  void* dst;
  const void* src;
  unsigned rows;
  unsigned esz;                           // bytes per element: 2, 4 or 8
  unsigned long long dst_row, dst_ch;     // strides of the batch's buffer, in elements
  unsigned long long src_row;             // row stride of the twin's buffer (its channel 0)
};

struct RestartTable
{
  RestartRegion r[kRestartMaxRegions];
  int n;
};

template <typename T>
__device__ inline void restart_copy(const RestartRegion& g, const int2* __restrict__ edits, unsigned n_edits,
                                    size_t i)
{
  const unsigned e = unsigned(i % n_edits);
  const unsigned row = unsigned(i / n_edits);
  const T v = static_cast<const T*>(g.src)[size_t(row) * g.src_row];
  static_cast<T*>(g.dst)[size_t(row) * g.dst_row + size_t(edits[e].x) * g.dst_ch] = v;
}

/* blockIdx.y < tab.n: region blockIdx.y for every edit (rows x edits elements, grid-stride over x);
 * blockIdx.y == tab.n: the tuner table rows, lut[c][0..T) = rows[edit's row][0..T). */
__global__ __launch_bounds__(256) void k_channel_restart(RestartTable tab, const int2* __restrict__ edits,
                                                         unsigned n_edits, const float2* __restrict__ lut_rows,
                                                         float2* __restrict__ lut, unsigned T)
{
  const size_t stride = size_t(gridDim.x) * blockDim.x;
  const size_t first = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (int(blockIdx.y) == tab.n)
  { // edit e's row j: threads of a wavefront cover consecutive table entries of one channel
    const size_t total = size_t(n_edits) * T;
    for (size_t i = first; i < total; i += stride)
    {
      const unsigned e = unsigned(i / T), j = unsigned(i % T);
      lut[size_t(edits[e].x) * T + j] = lut_rows[size_t(edits[e].y) * T + j];
    }
    return;
  }
  const RestartRegion g = tab.r[blockIdx.y];
  const size_t total = size_t(g.rows) * n_edits;
  for (size_t i = first; i < total; i += stride)
  {
    if (g.esz == 8)
      restart_copy<unsigned long long>(g, edits, n_edits, i);
    else if (g.esz == 4)
      restart_copy<unsigned>(g, edits, n_edits, i);
    else
      restart_copy<unsigned short>(g, edits, n_edits, i);
  }
}

/* k_channel_reset: cFmDecoder::Reset (FmDecode.cpp:326-338) of single channels at a call boundary
 * (fmd_batch_reset_channels).  Every region of a ResetTable is `rows` rows of CP elements of 4 or 8 bytes
 * (time-major state, channel stride 1); the host builds it from the list fmd_batch_reset's do_reset zeroes for
 * the whole batch (reset_regions, csrc/fmd_batch.hip).  The listed channels' elements become zero and their two
 * ring origins (the RDS low-pass's at origin[c], the matched filter's at origin[CP + c]) the batch's ring phases
 * at the next call's first sample, so that their rings start from slot 0 there like a freshly initialised
 * cFirFilter (FirFilter.cpp:330-377). */
constexpr int kResetMaxRegions = 40;

struct ResetRegion
{
  void* dst;
  unsigned rows;
  unsigned esz; // 4 or 8
};

struct ResetTable
{
  ResetRegion r[kResetMaxRegions];
  int n;
  unsigned CP;
  unsigned* origin;          // [2][CP]
  unsigned org_lpf, org_mf;  // what the listed channels' origins become
};

/* blockIdx.y < tab.n: region blockIdx.y for every listed channel (rows x channels elements, grid-stride over x);
 * blockIdx.y == tab.n: the origins.  channels[e].x is a listed channel (.y unused). */
__global__ __launch_bounds__(256) void k_channel_reset(ResetTable tab, const int2* __restrict__ channels,
                                                       unsigned n_ch)
{
  const size_t stride = size_t(gridDim.x) * blockDim.x;
  const size_t first = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (int(blockIdx.y) == tab.n)
  {
    for (size_t e = first; e < n_ch; e += stride)
    {
      const unsigned c = unsigned(channels[e].x);
      tab.origin[c] = tab.org_lpf;
      tab.origin[size_t(tab.CP) + c] = tab.org_mf;
    }
    return;
  }
  const ResetRegion g = tab.r[blockIdx.y];
  const size_t total = size_t(g.rows) * n_ch;
  for (size_t i = first; i < total; i += stride)
  {
    const size_t at = size_t(i / n_ch) * tab.CP + unsigned(channels[i % n_ch].x);
    if (g.esz == 8)
      static_cast<unsigned long long*>(g.dst)[at] = 0ull;
    else
      static_cast<unsigned*>(g.dst)[at] = 0u;
  }
}

} // namespace fmd
