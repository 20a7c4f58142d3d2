// Grouped aggregates: the predicate scan of query_scan.hip fused with an N-dimensional histogram
// (gfx950 / CDNA4, wave64).  One pass over the collection answers
// "SELECT c.x, c.y, COUNT(1), MIN(c.z) ... WHERE <filter> GROUP BY c.x, c.y": the host asks for the
// histogram of (x, y, z) dictionary ids over the selected rows and reduces it (ops/columnar.py
// reduce_hist).  The selection never leaves the registers: no mask and no row ids go to HBM.
//
// tt_scan_group: 0 to 3 key columns; the scan front end and the cell of a row are scan_cells.h's,
// shared with tt_scan_extrema and tt_scan_sums.  Counters are uint32, integer atomics
// only (deterministic): up to kMaxLdsGroups cells they are privatised in LDS and each block adds
// its non-zero cells to the output once, after its last tile; above that the rows add straight
// to the output.  Few cells (<= kSpreadCells: a boolean group, no group at all) would have the 64
// lanes of a wave add to a handful of LDS words, which the LDS serialises -- measured on MI355X
// at 1e8 selected rows, 2 groups: 0.217 ms against 0.096 ms for 200 groups.  Such a histogram is
// kept in kCopies interleaved copies (cell c of copy k at word c * kCopies + k, lane l adds to
// copy l mod kCopies: one bank per copy), summed per cell before the block's flush.
// The dynamic LDS holds the staged leaf bitmaps (when they fit) and, behind them, the histogram:
// at most 32 + 32 KiB.
#include "scan_cells.h"

namespace {
constexpr int kMaxLdsGroups = 8192;         // LDS-privatised counters (32 KiB), as tt_group_count
constexpr int64_t kMaxCells = 1 << 22;      // 16 MiB of counters; above it the host aggregates
}  // namespace

__global__ void __launch_bounds__(kScanBlock)
tt_scan_group(const ColumnDesc* __restrict__ cols,
              int64_t nrows, int64_t tiles,
              const uint16_t* __restrict__ live,      // 1 bit per row, row order
              const int32_t* __restrict__ prog, int32_t prog_len,
              const uint32_t* __restrict__ bitmaps, int32_t bitmap_words,
              GroupKeys gk, int32_t ncells,
              uint32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // [bitmaps | histogram], sized by the launcher
  const bool hist_lds = ncells <= kMaxLdsGroups;
  uint32_t* hist = stage_bitmaps(lds, bitmaps, bitmap_words);
  const uint32_t copies = hist_lds && ncells <= kSpreadCells ? kCopies : 1;
  if (hist_lds)
    for (int i = threadIdx.x; i < ncells * (int)copies; i += kScanBlock) hist[i] = 0;
  __syncthreads();
  uint32_t* cells = (hist_lds ? hist : counts) + (threadIdx.x & (copies - 1));  // this lane's copy
  scan_tiles(cols, nrows, tiles, live, prog, prog_len, bitmaps, bitmap_words, lds,
             [&](int64_t row0, uint32_t sel) __attribute__((always_inline)) {
               uint32_t cell[16];
               group_cells(cols, gk, row0, sel, cell);
#pragma unroll
               for (int i = 0; i < 16; ++i)
                 if ((sel >> i) & 1u) atomicAdd(&cells[cell[i] * copies], 1u);
             });
  if (hist_lds) {
    __syncthreads();
    for (int i = threadIdx.x; i < ncells; i += kScanBlock) {
      uint32_t sum = 0;
      for (uint32_t c = 0; c < copies; ++c) sum += hist[i * copies + c];
      if (sum) atomicAdd(&counts[i], sum);
    }
  }
}

// Preconditions (checked by the Python wrapper): as tt_launch_scan_eval, and every key column
// is a row of the column table.  `keys` / `dims`: host arrays of `nkeys` entries.  `counts`
// holds prod(dims[i] + 1) zeroed uint32.  `max_blocks`: 0 = as many blocks as stay resident
// (LDS per block against the CU's, at most 8 per CU).  -2: more cells than tt_group_max_cells().
extern "C" int tt_launch_scan_group(const void* cols, int64_t nrows, const uint16_t* live, const int32_t* prog,
                                    int32_t prog_len, const uint32_t* bitmaps, int32_t bitmap_words,
                                    const int32_t* keys, const int32_t* dims, int32_t nkeys, uint32_t* counts,
                                    int32_t max_blocks, hipStream_t stream) {
  if (prog_len <= 0 || nrows < 0 || bitmap_words <= 0 || max_blocks < 0) return -1;
  GroupKeys gk;
  int64_t ncells;
  if (const int rc = pack_keys(keys, dims, nkeys, kMaxGroupKeys, kMaxCells, gk, ncells)) return rc;
  const int64_t tiles = (nrows + kTileRows - 1) / kTileRows;
  if (tiles == 0) return 0;
  const size_t lds = bitmap_lds_bytes(bitmap_words) +
                     sizeof(uint32_t) * (ncells <= kSpreadCells ? (size_t)ncells * kCopies
                                         : ncells <= kMaxLdsGroups ? (size_t)ncells : 0);
  const int64_t blocks = resident_blocks(max_blocks, lds, tiles);
  if (blocks < 0) return (int)blocks;
  static bool lds_raised = false;  // bitmaps + histogram reach the 64 KiB default limit exactly
  if (const int rc = raise_dynamic_lds(reinterpret_cast<const void*>(tt_scan_group),
                                       sizeof(uint32_t) * (kMaxLdsBitmapWords + kMaxLdsGroups), lds_raised))
    return rc;
  hipLaunchKernelGGL(tt_scan_group, dim3((unsigned)blocks), dim3(kScanBlock), lds, stream,
                     reinterpret_cast<const ColumnDesc*>(cols), nrows, tiles, live, prog, prog_len, bitmaps,
                     bitmap_words, gk, (int32_t)ncells, counts);
  return (int)hipGetLastError();
}

extern "C" int tt_group_max_cells() { return (int)kMaxCells; }
