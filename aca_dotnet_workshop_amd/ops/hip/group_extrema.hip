// MIN / MAX / COUNT(key) per group in the scan pass (gfx950 / CDNA4, wave64): the sibling of
// tt_scan_group (group_agg.hip) for aggregate keys with too many distinct values for a histogram
// -- timestamps, one new dictionary value per write.  Three numbers per group instead of one
// counter per (group, value).
//
// tt_scan_extrema: the scan front end of tt_scan_group (persistent blocks over tiles, run_program
// over the lane's U 16-row groups, AND with liveness and row0 < nrows, leaf bitmaps staged in LDS
// when they fit) and its group cell: 0 to 2 group columns, axis i with dims[i] + 1 slots, slot
// dims[i] = "path missing", a row whose id is outside [0, dims[i]) and not missing is dropped.
// One value column: a row of the column table whose codes order as the values do (a rank-encoded
// copy, tt_rank_encode) and are compared as unsigned 32-bit integers; the all-ones code of its
// width (-1 after load16) = undefined.  For every selected, non-dropped row with a defined value:
//   counts[cell] += 1;  lo[cell] = min(lo[cell], code << 32 | row);  hi[cell] = max(hi[cell], same)
// The caller initialises counts = 0, lo = all-ones, hi = 0; lo / hi of a cell mean something only
// where counts > 0.  The row under the code lets the host turn an extremum back into a value with
// one ids[col, row] lookup per group; ties on the code go to the lowest / highest row.
// Integer atomics only (deterministic).  Three instantiations, chosen by the launcher:
//   kOneCell   no group column: the lane reduces its rows in registers over all its tiles, the
//              wave reduces across lanes (shuffles), one lane per wave merges into LDS.
//   kLdsCells  up to kMaxLdsCells cells privatised in LDS (8 + 8 + 4 bytes per cell), flushed once
//              per block after its last tile.  Up to kSpreadCells cells (a boolean group) are kept
//              in kCopies interleaved copies, lane l on copy l mod kCopies, as tt_scan_group keeps
//              its few-cell histograms: 64 lanes do not queue on a handful of LDS words.
//   kGlobalCells  above that, up to tt_group_max_cells(): the rows update the output directly.
// Most rows do not improve an extremum: the current lo / hi is read first (one untorn 64-bit
// load) and the atomic skipped when the row cannot win.  lo only falls and hi only rises, so a
// stale read costs a redundant atomic, never a wrong result.
// Dynamic LDS: [bitmaps | lo | hi | counts], at most 32 + 80 KiB of the CU's 160.
#include "scan_common.h"

extern "C" int tt_group_max_cells();  // group_agg.hip: the cell cap is the histogram's

namespace {
constexpr int kExtU = 2;                    // row groups per lane, as tt_scan_group
constexpr int kExtBlock = kTileRows / (kRowsPerLane * kExtU);
constexpr int kExtMaxKeys = 2;
constexpr int kMaxLdsCells = 4096;          // 20 B each: 80 KiB
constexpr int kSpreadCells = 64;            // up to here kCopies interleaved copies
constexpr int kCopies = 32;
constexpr int kCellBytes = 20;
constexpr int kLdsBudget = 160 * 1024;      // LDS per CU: bounds the resident blocks
constexpr uint64_t kNoLo = ~0ull;

enum ExtMode : int { kOneCell = 0, kLdsCells = 1, kGlobalCells = 2 };

struct ExtKeys {
  int32_t col[kExtMaxKeys];
  int32_t dim[kExtMaxKeys];
  int32_t nkeys;
  int32_t vcol;
};

// n rows with keys in [klo, khi] into slot idx.  LDS: workgroup scope; the output: agent scope.
template <bool LDS>
__device__ __forceinline__ void merge(uint32_t* cnt, uint64_t* lo, uint64_t* hi, uint32_t idx, uint32_t n,
                                      uint64_t klo, uint64_t khi) {
  constexpr int scope = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
  __hip_atomic_fetch_add(cnt + idx, n, __ATOMIC_RELAXED, scope);
  if (klo < __hip_atomic_load(lo + idx, __ATOMIC_RELAXED, scope))
    __hip_atomic_fetch_min(lo + idx, klo, __ATOMIC_RELAXED, scope);
  if (khi > __hip_atomic_load(hi + idx, __ATOMIC_RELAXED, scope))
    __hip_atomic_fetch_max(hi + idx, khi, __ATOMIC_RELAXED, scope);
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int mask) {
  return (uint64_t)__shfl_xor((unsigned long long)v, mask, 64);
}
}  // namespace

template <int MODE>
__global__ void __launch_bounds__(kExtBlock)
tt_scan_extrema(const ColumnDesc* __restrict__ cols,
                int64_t nrows, int64_t tiles,
                const uint16_t* __restrict__ live,      // 1 bit per row, row order
                const int32_t* __restrict__ prog, int32_t prog_len,
                const uint32_t* __restrict__ bitmaps, int32_t bitmap_words,
                ExtKeys gk, int32_t ncells,
                uint32_t* __restrict__ counts, uint64_t* __restrict__ lo, uint64_t* __restrict__ hi) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // [bitmaps | lo | hi | counts], sized by the launcher
  const bool in_lds = bitmap_words <= kMaxLdsBitmapWords;
  const uint32_t copies = (MODE == kLdsCells && ncells <= kSpreadCells) ? kCopies : 1;
  const int slots = MODE == kGlobalCells ? 0 : ncells * (int)copies;
  uint64_t* s_lo = reinterpret_cast<uint64_t*>(lds + (in_lds ? (bitmap_words + 3) & ~3 : 0));  // 16-byte aligned
  uint64_t* s_hi = s_lo + slots;
  uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_hi + slots);
  if (in_lds)
    for (int i = threadIdx.x; i < bitmap_words; i += kExtBlock) lds[i] = bitmaps[i];
  for (int i = threadIdx.x; i < slots; i += kExtBlock) {
    s_lo[i] = kNoLo;
    s_hi[i] = 0;
    s_cnt[i] = 0;
  }
  __syncthreads();
  const uint32_t copy = threadIdx.x & (copies - 1);  // this lane's copy
  uint32_t a_cnt = 0;                                // kOneCell: the lane's own reduction
  uint64_t a_lo = kNoLo, a_hi = 0;
  const ColumnDesc vcd = cols[gk.vcol];
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int64_t row0[kExtU];
    uint16_t lv[kExtU];
#pragma unroll
    for (int u = 0; u < kExtU; ++u) {
      row0[u] = tile * kTileRows + (int64_t)u * (kExtBlock * kRowsPerLane) + (int64_t)threadIdx.x * kRowsPerLane;
      lv[u] = live[row0[u] >> 4];
    }
    uint32_t m[kExtU];
    if (in_lds) run_program<kExtU>(cols, prog, prog_len, (const uint32_t*)lds, row0, m);
    else run_program<kExtU>(cols, prog, prog_len, bitmaps, row0, m);
#pragma unroll
    for (int u = 0; u < kExtU; ++u) {
      uint32_t sel = row0[u] < nrows ? (m[u] & (uint32_t)lv[u]) : 0u;
      if (!sel) continue;
      int32_t val[16];
      load16(vcd, row0[u], val);
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (val[i] == -1) sel &= ~(1u << i);  // undefined: counts nowhere
      const uint64_t rowbase = (uint64_t)row0[u];  // < 2^32 (launcher)
      if constexpr (MODE == kOneCell) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if (!((sel >> i) & 1u)) continue;
          const uint64_t key = ((uint64_t)(uint32_t)val[i] << 32) | (rowbase + i);
          a_cnt += 1;
          a_lo = key < a_lo ? key : a_lo;
          a_hi = key > a_hi ? key : a_hi;
        }
      } else {
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
        for (int i = 0; i < 16; ++i) {
          if (!((sel >> i) & 1u)) continue;
          const uint64_t key = ((uint64_t)(uint32_t)val[i] << 32) | (rowbase + i);
          if constexpr (MODE == kLdsCells) merge<true>(s_cnt, s_lo, s_hi, cell[i] * copies + copy, 1u, key, key);
          else merge<false>(counts, lo, hi, cell[i], 1u, key, key);
        }
      }
    }
  }
  if constexpr (MODE == kOneCell) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t c = (uint32_t)__shfl_xor((int)a_cnt, off, 64);
      const uint64_t l = shfl_xor64(a_lo, off), h = shfl_xor64(a_hi, off);
      a_cnt += c;
      a_lo = l < a_lo ? l : a_lo;
      a_hi = h > a_hi ? h : a_hi;
    }
    if ((threadIdx.x & 63) == 0 && a_cnt) merge<true>(s_cnt, s_lo, s_hi, 0u, a_cnt, a_lo, a_hi);
  }
  if constexpr (MODE != kGlobalCells) {
    __syncthreads();
    for (int i = threadIdx.x; i < ncells; i += kExtBlock) {
      uint32_t sum = 0;
      uint64_t l = kNoLo, h = 0;
      for (uint32_t c = 0; c < copies; ++c) {
        const uint32_t s = i * copies + c;
        sum += s_cnt[s];
        l = s_lo[s] < l ? s_lo[s] : l;
        h = s_hi[s] > h ? s_hi[s] : h;
      }
      if (sum) merge<false>(counts, lo, hi, (uint32_t)i, sum, l, h);
    }
  }
}

namespace {
template <int MODE>
int launch_extrema(int64_t blocks, size_t lds, hipStream_t stream, const void* cols, int64_t nrows, int64_t tiles,
                   const uint16_t* live, const int32_t* prog, int32_t prog_len, const uint32_t* bitmaps,
                   int32_t bitmap_words, const ExtKeys& gk, int32_t ncells, uint32_t* counts, uint64_t* lo,
                   uint64_t* hi) {
  hipLaunchKernelGGL(tt_scan_extrema<MODE>, dim3((unsigned)blocks), dim3(kExtBlock), lds, stream,
                     reinterpret_cast<const ColumnDesc*>(cols), nrows, tiles, live, prog, prog_len, bitmaps,
                     bitmap_words, gk, ncells, counts, lo, hi);
  return (int)hipGetLastError();
}
}  // namespace

// Preconditions (checked by the Python wrapper): as tt_launch_scan_group, and `value_col` is a
// row of the column table.  `counts` / `lo` / `hi` hold prod(dims[i] + 1) cells, initialised to
// 0 / all-ones / 0.  nrows <= 2^32: the row shares a word with the code.  `max_blocks`: 0 = as
// many blocks as stay resident (LDS per block against the CU's, at most 8 per CU).
// -2: more cells than tt_group_max_cells().  Nothing is launched on a refusal.
extern "C" int tt_launch_scan_extrema(const void* cols, int64_t nrows, const uint16_t* live, const int32_t* prog,
                                      int32_t prog_len, const uint32_t* bitmaps, int32_t bitmap_words,
                                      const int32_t* keys, const int32_t* dims, int32_t nkeys, int32_t value_col,
                                      uint32_t* counts, uint64_t* lo, uint64_t* hi, int32_t max_blocks,
                                      hipStream_t stream) {
  if (prog_len <= 0 || nrows < 0 || nrows > (int64_t)1 << 32 || bitmap_words <= 0 || nkeys < 0 ||
      nkeys > kExtMaxKeys || value_col < 0 || max_blocks < 0)
    return -1;
  ExtKeys gk = {};
  gk.nkeys = nkeys;
  gk.vcol = value_col;
  int64_t ncells = 1;
  for (int i = 0; i < nkeys; ++i) {
    if (keys[i] < 0 || dims[i] < 0) return -1;
    gk.col[i] = keys[i];
    gk.dim[i] = dims[i];
    ncells *= (int64_t)dims[i] + 1;
    if (ncells > tt_group_max_cells()) return -2;
  }
  const int64_t tiles = (nrows + kTileRows - 1) / kTileRows;
  if (tiles == 0) return 0;
  const int mode = nkeys == 0 ? kOneCell : ncells <= kMaxLdsCells ? kLdsCells : kGlobalCells;
  const size_t slots = mode == kGlobalCells ? 0 : mode == kLdsCells && ncells <= kSpreadCells ? (size_t)ncells * kCopies
                                                                                              : (size_t)ncells;
  const size_t lds = sizeof(uint32_t) * (bitmap_words <= kMaxLdsBitmapWords ? (size_t)((bitmap_words + 3) & ~3) : 0) +
                     kCellBytes * slots;
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
  static bool lds_raised = false;  // bitmaps + cells go past the 64 KiB default limit
  if (mode == kLdsCells && !lds_raised) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(tt_scan_extrema<kLdsCells>),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            sizeof(uint32_t) * kMaxLdsBitmapWords + kCellBytes * kMaxLdsCells) != hipSuccess)
      return -4;
    lds_raised = true;
  }
  if (mode == kOneCell)
    return launch_extrema<kOneCell>(blocks, lds, stream, cols, nrows, tiles, live, prog, prog_len, bitmaps,
                                    bitmap_words, gk, (int32_t)ncells, counts, lo, hi);
  if (mode == kLdsCells)
    return launch_extrema<kLdsCells>(blocks, lds, stream, cols, nrows, tiles, live, prog, prog_len, bitmaps,
                                     bitmap_words, gk, (int32_t)ncells, counts, lo, hi);
  return launch_extrema<kGlobalCells>(blocks, lds, stream, cols, nrows, tiles, live, prog, prog_len, bitmaps,
                                      bitmap_words, gk, (int32_t)ncells, counts, lo, hi);
}

extern "C" int tt_extrema_max_lds_cells() { return kMaxLdsCells; }
