// What the grouped-aggregate kernels share (group_agg.hip tt_scan_group, group_extrema.hip
// tt_scan_extrema, group_sums.hip tt_scan_sums, and through sparse_cells.h their hashed siblings
// and group_sparse.hip tt_scan_sparse; gfx950 / CDNA4, wave64): the scan front end, the
// cell of a row and the launchers' key packing and grid sizing.  ops/columnar.py (cells_of) and the
// stand-in device of the tests compute the same cell on the host.
//
// Front end: persistent blocks, block b evaluates tiles b, b + blocks, ... exactly as
// tt_scan_eval_t does (run_program over the lane's kScanU 16-row groups, AND with liveness and
// row0 < nrows); the leaf bitmaps are staged in LDS when they fit.  The selection never leaves the
// registers: no mask and no row ids go to HBM, and only groups with a selected row load their key
// and value columns.
// Cell: axis i of the key columns has dims[i] + 1 slots, slot dims[i] = "path missing"; the cell of
// a row is (s0 * (n1+1) + s1) * (n2+1) + s2, one cell with no key.  A row whose id is outside
// [0, dims[i]) and not the missing code (a dictionary that grew after the host read its size, a
// stray 4-byte value) is dropped.
#pragma once
#include "scan_common.h"

namespace {
constexpr int kScanU = 2;                   // row groups per lane, as tt_scan_eval (kEvalGroups)
constexpr int kScanBlock = kTileRows / (kRowsPerLane * kScanU);
constexpr int kMaxGroupKeys = 3;            // the histogram's; the value kernels take 2
constexpr int kSpreadCells = 64;            // up to here cells in LDS are kept in kCopies interleaved copies
constexpr int kCopies = 32;                 // one per LDS bank
constexpr int kLdsBudget = 160 * 1024;      // LDS per CU: bounds the resident blocks

struct GroupKeys {
  int32_t col[kMaxGroupKeys];
  int32_t dim[kMaxGroupKeys];
  int32_t nkeys;
  int32_t vcol;  // the value column (tt_scan_group has none)
};

// Copies the leaf bitmaps to the front of the dynamic LDS when they fit (visible after the
// caller's __syncthreads) and returns the first 16-byte aligned word behind them.
__device__ __forceinline__ uint32_t* stage_bitmaps(uint32_t* lds, const uint32_t* __restrict__ bitmaps,
                                                   int32_t bitmap_words) {
  if (bitmap_words > kMaxLdsBitmapWords) return lds;
  for (int i = threadIdx.x; i < bitmap_words; i += kScanBlock) lds[i] = bitmaps[i];
  return lds + ((bitmap_words + 3) & ~3);
}

// The block's tiles: each(row0, sel) for every 16-row group of this lane with a selected row,
// bit i of sel = row row0 + i.  `lds`: where stage_bitmaps put the bitmaps.  STOP (the hashed
// kernels, sparse_cells.h): `*stop` is read before each tile and the scan ends once it is set.
template <bool STOP = false, typename Each>
__device__ __forceinline__ void scan_tiles(const ColumnDesc* __restrict__ cols, int64_t nrows, int64_t tiles,
                                           const uint16_t* __restrict__ live,  // 1 bit per row, row order
                                           const int32_t* __restrict__ prog, int32_t prog_len,
                                           const uint32_t* __restrict__ bitmaps, int32_t bitmap_words,
                                           const uint32_t* lds, Each each, const uint32_t* stop = nullptr) {
  const bool in_lds = bitmap_words <= kMaxLdsBitmapWords;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    if constexpr (STOP)
      if (__hip_atomic_load(stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
    int64_t row0[kScanU];
    uint16_t lv[kScanU];
#pragma unroll
    for (int u = 0; u < kScanU; ++u) {
      row0[u] = tile * kTileRows + (int64_t)u * (kScanBlock * kRowsPerLane) + (int64_t)threadIdx.x * kRowsPerLane;
      lv[u] = live[row0[u] >> 4];
    }
    uint32_t m[kScanU];
    if (in_lds) run_program<kScanU>(cols, prog, prog_len, lds, row0, m);
    else run_program<kScanU>(cols, prog, prog_len, bitmaps, row0, m);
#pragma unroll
    for (int u = 0; u < kScanU; ++u) {
      const uint32_t sel = row0[u] < nrows ? (m[u] & (uint32_t)lv[u]) : 0u;
      if (sel) each(row0[u], sel);
    }
  }
}

// The cells of rows [row0, row0 + 16); clears the sel bit of a dropped row.
__device__ __forceinline__ void group_cells(const ColumnDesc* __restrict__ cols, const GroupKeys& gk, int64_t row0,
                                            uint32_t& sel, uint32_t (&cell)[16]) {
#pragma unroll
  for (int i = 0; i < 16; ++i) cell[i] = 0;
  for (int j = 0; j < gk.nkeys; ++j) {
    const uint32_t n = (uint32_t)gk.dim[j];
    int32_t ids[16];
    load16(cols[gk.col[j]], row0, ids);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const bool missing = ids[i] == -1;
      const uint32_t slot = missing ? n : (uint32_t)ids[i];  // other negatives: far above n
      if (!missing && slot >= n) sel &= ~(1u << i);
      cell[i] = cell[i] * (n + 1u) + slot;  // wraps only for dropped rows
    }
  }
}

// `keys` / `dims` (host arrays of `nkeys` entries) into gk, ncells = prod(dims[i] + 1).
// -1: a bad argument; -2: more cells than `max_cells`.
inline int pack_keys(const int32_t* keys, const int32_t* dims, int32_t nkeys, int max_keys, int64_t max_cells,
                     GroupKeys& gk, int64_t& ncells) {
  if (nkeys < 0 || nkeys > max_keys) return -1;
  gk = {};
  gk.nkeys = nkeys;
  ncells = 1;
  for (int i = 0; i < nkeys; ++i) {
    if (keys[i] < 0 || dims[i] < 0) return -1;
    gk.col[i] = keys[i];
    gk.dim[i] = dims[i];
    ncells *= (int64_t)dims[i] + 1;
    if (ncells > max_cells) return -2;
  }
  return 0;
}

// Dynamic LDS that stage_bitmaps takes.
inline size_t bitmap_lds_bytes(int32_t bitmap_words) {
  return sizeof(uint32_t) * (bitmap_words <= kMaxLdsBitmapWords ? (size_t)((bitmap_words + 3) & ~3) : 0);
}

// The grid: `max_blocks`, or with 0 as many blocks as stay resident (`lds` bytes per block against
// the CU's, 1 to 8 per CU); never more than the tiles.  -3: the device does not tell its CUs.
inline int64_t resident_blocks(int32_t max_blocks, size_t lds, int64_t tiles) {
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
  return blocks > tiles ? tiles : blocks;
}

// Lets `kernel` take `bytes` of dynamic LDS (the default limit is 64 KiB), once.  -4: refused.
inline int raise_dynamic_lds(const void* kernel, size_t bytes, bool& raised) {
  if (raised) return 0;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return -4;
  raised = true;
  return 0;
}
}  // namespace
