// Grouped aggregates: the predicate scan of query_scan.hip fused with an N-dimensional histogram
// (gfx950 / CDNA4, wave64).  One pass over the collection answers
// "SELECT c.x, c.y, COUNT(1), MIN(c.z) ... WHERE <filter> GROUP BY c.x, c.y": the host asks for the
// histogram of (x, y, z) dictionary ids over the selected rows and reduces it (ops/columnar.py
// reduce_hist).  The selection never leaves the registers: no mask and no row ids go to HBM.
//
// tt_scan_group: 0 to 3 key columns.  Axis i has dims[i] + 1 slots, slot dims[i] = "path
// missing"; the cell of a row is (s0 * (n1+1) + s1) * (n2+1) + s2, one cell with no key.  A row
// whose id is outside [0, dims[i]) and not the missing code (a dictionary that grew after the
// host read its size, a stray 4-byte value) is dropped.
// Persistent blocks: block b evaluates tiles b, b + blocks, ... exactly as tt_scan_eval_t does
// (run_program over the lane's U 16-row groups, AND with liveness and row0 < nrows); only groups
// with a selected row load their key columns' 16 codes.  Counters are uint32, integer atomics
// only (deterministic): up to kMaxLdsGroups cells they are privatised in LDS and each block adds
// its non-zero cells to the output once, after its last tile; above that the rows add straight
// to the output.  Few cells (<= kSpreadCells: a boolean group, no group at all) would have the 64
// lanes of a wave add to a handful of LDS words, which the LDS serialises -- measured on MI355X
// at 1e8 selected rows, 2 groups: 0.217 ms against 0.096 ms for 200 groups.  Such a histogram is
// kept in kCopies interleaved copies (cell c of copy k at word c * kCopies + k, lane l adds to
// copy l mod kCopies: one bank per copy), summed per cell before the block's flush.
// The dynamic LDS holds the staged leaf bitmaps (when they fit) and, behind them, the histogram:
// at most 32 + 32 KiB.
#include "scan_common.h"

namespace {
constexpr int kGroupU = 2;                  // row groups per lane, as tt_scan_eval (kEvalGroups)
constexpr int kGroupBlock = kTileRows / (kRowsPerLane * kGroupU);
constexpr int kMaxKeys = 3;
constexpr int kMaxLdsGroups = 8192;         // LDS-privatised counters (32 KiB), as tt_group_count
constexpr int64_t kMaxCells = 1 << 22;      // 16 MiB of counters; above it the host aggregates
constexpr int kSpreadCells = 64;            // up to here the LDS histogram is kept in kCopies copies
constexpr int kCopies = 32;                 // one per LDS bank
constexpr int kLdsBudget = 160 * 1024;      // LDS per CU: bounds the resident blocks

struct GroupKeys {
  int32_t col[kMaxKeys];
  int32_t dim[kMaxKeys];
  int32_t nkeys;
};
}  // namespace

__global__ void __launch_bounds__(kGroupBlock)
tt_scan_group(const ColumnDesc* __restrict__ cols,
              int64_t nrows, int64_t tiles,
              const uint16_t* __restrict__ live,      // 1 bit per row, row order
              const int32_t* __restrict__ prog, int32_t prog_len,
              const uint32_t* __restrict__ bitmaps, int32_t bitmap_words,
              GroupKeys gk, int32_t ncells,
              uint32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // [bitmaps | histogram], sized by the launcher
  const bool in_lds = bitmap_words <= kMaxLdsBitmapWords;
  const bool hist_lds = ncells <= kMaxLdsGroups;
  uint32_t* hist = lds + (in_lds ? (bitmap_words + 3) & ~3 : 0);
  if (in_lds)
    for (int i = threadIdx.x; i < bitmap_words; i += kGroupBlock) lds[i] = bitmaps[i];
  const uint32_t copies = hist_lds && ncells <= kSpreadCells ? kCopies : 1;
  if (hist_lds)
    for (int i = threadIdx.x; i < ncells * (int)copies; i += kGroupBlock) hist[i] = 0;
  __syncthreads();
  uint32_t* cells = (hist_lds ? hist : counts) + (threadIdx.x & (copies - 1));  // this lane's copy
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int64_t row0[kGroupU];
    uint16_t lv[kGroupU];
#pragma unroll
    for (int u = 0; u < kGroupU; ++u) {
      row0[u] = tile * kTileRows + (int64_t)u * (kGroupBlock * kRowsPerLane) + (int64_t)threadIdx.x * kRowsPerLane;
      lv[u] = live[row0[u] >> 4];
    }
    uint32_t m[kGroupU];
    if (in_lds) run_program<kGroupU>(cols, prog, prog_len, (const uint32_t*)lds, row0, m);
    else run_program<kGroupU>(cols, prog, prog_len, bitmaps, row0, m);
#pragma unroll
    for (int u = 0; u < kGroupU; ++u) {
      uint32_t sel = row0[u] < nrows ? (m[u] & (uint32_t)lv[u]) : 0u;
      if (!sel) continue;
      uint32_t cell[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) cell[i] = 0;
      for (int j = 0; j < gk.nkeys; ++j) {
        const uint32_t n = (uint32_t)gk.dim[j];
        int32_t ids[16];
        load16(cols[gk.col[j]], row0[u], ids);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const bool missing = ids[i] == -1;
          const uint32_t slot = missing ? n : (uint32_t)ids[i];  // other negatives: far above n
          if (!missing && slot >= n) sel &= ~(1u << i);
          cell[i] = cell[i] * (n + 1u) + slot;  // wraps only for dropped rows
        }
      }
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if ((sel >> i) & 1u) atomicAdd(&cells[cell[i] * copies], 1u);
    }
  }
  if (hist_lds) {
    __syncthreads();
    for (int i = threadIdx.x; i < ncells; i += kGroupBlock) {
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
  if (prog_len <= 0 || nrows < 0 || bitmap_words <= 0 || nkeys < 0 || nkeys > kMaxKeys || max_blocks < 0) return -1;
  GroupKeys gk = {};
  gk.nkeys = nkeys;
  int64_t ncells = 1;
  for (int i = 0; i < nkeys; ++i) {
    if (keys[i] < 0 || dims[i] < 0) return -1;
    gk.col[i] = keys[i];
    gk.dim[i] = dims[i];
    ncells *= (int64_t)dims[i] + 1;
    if (ncells > kMaxCells) return -2;
  }
  const int64_t tiles = (nrows + kTileRows - 1) / kTileRows;
  if (tiles == 0) return 0;
  const size_t lds = sizeof(uint32_t) * ((bitmap_words <= kMaxLdsBitmapWords ? (size_t)((bitmap_words + 3) & ~3) : 0) +
                                         (ncells <= kSpreadCells ? (size_t)ncells * kCopies
                                          : ncells <= kMaxLdsGroups ? (size_t)ncells : 0));
  int64_t blocks = max_blocks;
  if (blocks == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      return -3;
    int per_cu = lds ? (int)(kLdsBudget / lds) : 8;
    per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;
    blocks = (int64_t)cus * per_cu;
  }
  if (blocks > tiles) blocks = tiles;
  static bool lds_raised = false;  // bitmaps + histogram reach the 64 KiB default limit exactly
  if (!lds_raised) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(tt_scan_group), hipFuncAttributeMaxDynamicSharedMemorySize,
                            sizeof(uint32_t) * (kMaxLdsBitmapWords + kMaxLdsGroups)) != hipSuccess)
      return -4;
    lds_raised = true;
  }
  hipLaunchKernelGGL(tt_scan_group, dim3((unsigned)blocks), dim3(kGroupBlock), lds, stream,
                     reinterpret_cast<const ColumnDesc*>(cols), nrows, tiles, live, prog, prog_len, bitmaps,
                     bitmap_words, gk, (int32_t)ncells, counts);
  return (int)hipGetLastError();
}

extern "C" int tt_group_max_cells() { return (int)kMaxCells; }
