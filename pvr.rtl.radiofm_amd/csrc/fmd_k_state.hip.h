/*
 * fmd_k_state.hip.h -- k_channel_export / k_channel_import: the carried state of single channels out of a batch and
 * into one (fmd_batch_save_state / _load_state / _export_channels / _import_channels).
 *
 * The regions are those of a restart (fmd_k_restart.hip.h) plus the status record and the clip counter: one buffer of
 * per-channel state each, `rows` elements per channel of 2, 4 or 8 bytes, element (row, c) at
 * base + row * row_stride + c * ch_stride (in elements; the channel-major IF history has the strides swapped).
 * Outside the batch a region is packed row-major over the n channels of a blob, [row][n] -- the batch's own [row][CP]
 * with n in place of CP -- at byte offset `off` * n of the payload (`off`: the bytes per channel of the regions in
 * front, each rounded up to 8, so every region starts aligned whatever n is).
 *
 * Consecutive threads take consecutive list entries of one (region, row): both sides of the copy coalesce where the
 * listed channels are neighbours (a whole batch: always; an import's list comes sorted by channel).
 */
#pragma once

#include "fmd_k_common.hip.h"

namespace fmd
{

constexpr int kStateMaxRegions = 40;

struct StateRegion
{
  void* base;
  unsigned rows;
  unsigned esz;                   // bytes per element: 2, 4 or 8
  unsigned long long row, ch;     // strides of the batch's buffer, in elements
  unsigned long long off;         // byte offset of the region in a one-channel payload
};

struct StateTable
{
  StateRegion r[kStateMaxRegions];
  int n;
};

/* one list entry: channel of the batch, column of the payload, row of the staged tuner table (imports) */
struct StateEdit
{
  int ch, col, lut_row, pad;
};

template <typename T>
__device__ inline T* state_packed(const StateRegion& g, void* payload, unsigned n_cols, unsigned row, unsigned col)
{
  return reinterpret_cast<T*>(static_cast<char*>(payload) + g.off * n_cols) + size_t(row) * n_cols + col;
}

template <typename T, bool IMPORT>
__device__ inline void state_copy(const StateRegion& g, const StateEdit* __restrict__ list, unsigned n_list,
                                  void* payload, unsigned n_cols, unsigned col0, size_t i)
{
  const unsigned e = unsigned(i % n_list);
  const unsigned row = unsigned(i / n_list);
  // no list: channel e of the batch is column col0 + e (a whole batch, or a sub-batch of one)
  const unsigned ch = list ? unsigned(list[e].ch) : e;
  const unsigned col = list ? unsigned(list[e].col) : col0 + e;
  T* inside = static_cast<T*>(g.base) + size_t(row) * g.row + size_t(ch) * g.ch;
  T* packed = state_packed<T>(g, payload, n_cols, row, col);
  if (IMPORT)
    *inside = *packed;
  else
    *packed = *inside;
}

template <bool IMPORT>
__device__ inline void state_walk(const StateTable& tab, const StateEdit* __restrict__ list, unsigned n_list,
                                  void* payload, unsigned n_cols, unsigned col0)
{
  const size_t stride = size_t(gridDim.x) * blockDim.x;
  const size_t first = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const StateRegion g = tab.r[blockIdx.y];
  const size_t total = size_t(g.rows) * n_list;
  for (size_t i = first; i < total; i += stride)
  {
    if (g.esz == 8)
      state_copy<unsigned long long, IMPORT>(g, list, n_list, payload, n_cols, col0, i);
    else if (g.esz == 4)
      state_copy<unsigned, IMPORT>(g, list, n_list, payload, n_cols, col0, i);
    else
      state_copy<unsigned short, IMPORT>(g, list, n_list, payload, n_cols, col0, i);
  }
}

/* blockIdx.y = region: the listed channels' elements into the packed rows (grid-stride over x) */
__global__ __launch_bounds__(256) void k_channel_export(StateTable tab, const StateEdit* __restrict__ list,
                                                        unsigned n_list, void* __restrict__ payload, unsigned n_cols,
                                                        unsigned col0)
{
  state_walk<false>(tab, list, n_list, payload, n_cols, col0);
}

/* blockIdx.y < tab.n: region blockIdx.y, the packed rows into the listed channels; blockIdx.y == tab.n: the tuner
 * table rows, lut[c][0..T) = lut_rows[entry's row][0..T) (k_channel_restart's walk; lut_rows null: none) */
__global__ __launch_bounds__(256) void k_channel_import(StateTable tab, const StateEdit* __restrict__ list,
                                                        unsigned n_list, const void* __restrict__ payload,
                                                        unsigned n_cols, unsigned col0,
                                                        const float2* __restrict__ lut_rows, float2* __restrict__ lut,
                                                        unsigned T)
{
  if (int(blockIdx.y) == tab.n)
  {
    if (!lut_rows || !list)
      return;
    const size_t stride = size_t(gridDim.x) * blockDim.x;
    const size_t total = size_t(n_list) * T;
    for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += stride)
    {
      const unsigned e = unsigned(i / T), j = unsigned(i % T);
      lut[size_t(list[e].ch) * T + j] = lut_rows[size_t(list[e].lut_row) * T + j];
    }
    return;
  }
  state_walk<true>(tab, list, n_list, const_cast<void*>(payload), n_cols, col0);
}

} // namespace fmd
