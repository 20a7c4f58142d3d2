// Exact SUM / AVG(key) per group in the scan pass (gfx950 / CDNA4, wave64): the sibling of
// tt_scan_extrema (group_extrema.hip) for numeric aggregate keys with too many distinct values for
// a histogram -- amounts, durations, points, about one dictionary value per row.
//
// The numbers of a column share a power-of-two quantum 2^e (Column.num_scale, ops/columnar.py):
// every float(v) is m * 2^e with an integer m.  The host keeps the m of every dictionary id in one
// int64 table (INT64_MIN = the id's value is no number); the kernel gathers m = nums[id] for every
// selected row and adds integers, so the result does not depend on the order the rows arrive in:
//   cnt[cell] += 1;  sum[cell] += m (int64);  abs[cell] += |m| (uint64)
// abs < 2^53 proves to the host that the correctly rounded sum of the doubles is sum * 2^e exactly
// (AggGroups, ops/columnar.py); the caller guarantees max|m| * rows < 2^63, so neither word wraps.
//
// tt_scan_sums: the scan front end and the group cell of tt_scan_extrema -- persistent blocks over
// tiles, run_program over the lane's U 16-row groups, AND with liveness and row0 < nrows, leaf
// bitmaps staged in LDS when they fit; 0 to 2 group columns, axis i with dims[i] + 1 slots, slot
// dims[i] = "path missing", a row whose id is outside [0, dims[i]) and not missing is dropped.
// The value column is the key's own id column (any width); a row whose id is missing, at or past
// `nvalues`, or whose m is INT64_MIN adds nothing.  The caller zeroes cnt / sum / abs.
// Three instantiations with the sibling's thresholds, chosen by the launcher:
//   kOneCell   no group column: the lane adds its rows in registers over all its tiles, the wave
//              adds across lanes (shuffles), one lane per wave merges into LDS.
//   kLdsCells  up to kMaxLdsCells cells privatised in LDS (8 + 8 + 4 bytes per cell), flushed once
//              per block after its last tile; up to kSpreadCells cells in kCopies interleaved
//              copies, lane l on copy l mod kCopies.
//   kGlobalCells  above that, up to tt_group_max_cells(): 64-bit integer atomics on the output.
// Dynamic LDS: [bitmaps | sum | abs | cnt], at most 32 + 80 KiB of the CU's 160.
#include "scan_common.h"

extern "C" int tt_group_max_cells();  // group_agg.hip: the cell cap is the histogram's

namespace {
constexpr int kSumU = 2;                    // row groups per lane, as tt_scan_group
constexpr int kSumBlock = kTileRows / (kRowsPerLane * kSumU);
constexpr int kSumMaxKeys = 2;
constexpr int kSumMaxLdsCells = 4096;       // 20 B each: 80 KiB
constexpr int kSumSpreadCells = 64;         // up to here kSumCopies interleaved copies
constexpr int kSumCopies = 32;
constexpr int kSumCellBytes = 20;
constexpr int kSumLdsBudget = 160 * 1024;   // LDS per CU: bounds the resident blocks
constexpr int64_t kNoNumber = INT64_MIN;

enum SumMode : int { kOneCell = 0, kLdsCells = 1, kGlobalCells = 2 };

struct SumKeys {
  int32_t col[kSumMaxKeys];
  int32_t dim[kSumMaxKeys];
  int32_t nkeys;
  int32_t vcol;
};

// n numbers with sum s and sum of magnitudes a into slot idx.  LDS: workgroup scope; the output:
// agent scope.  The signed sum is added as its two's complement word.
template <bool LDS>
__device__ __forceinline__ void merge(uint32_t* cnt, uint64_t* sum, uint64_t* abs, uint32_t idx, uint32_t n,
                                      uint64_t s, uint64_t a) {
  constexpr int scope = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
  __hip_atomic_fetch_add(cnt + idx, n, __ATOMIC_RELAXED, scope);
  __hip_atomic_fetch_add(sum + idx, s, __ATOMIC_RELAXED, scope);
  __hip_atomic_fetch_add(abs + idx, a, __ATOMIC_RELAXED, scope);
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int mask) {
  return (uint64_t)__shfl_xor((unsigned long long)v, mask, 64);
}
}  // namespace

template <int MODE>
__global__ void __launch_bounds__(kSumBlock)
tt_scan_sums(const ColumnDesc* __restrict__ cols,
             int64_t nrows, int64_t tiles,
             const uint16_t* __restrict__ live,      // 1 bit per row, row order
             const int32_t* __restrict__ prog, int32_t prog_len,
             const uint32_t* __restrict__ bitmaps, int32_t bitmap_words,
             SumKeys gk, int32_t ncells,
             const int64_t* __restrict__ nums, uint32_t nvalues,   // id -> m
             uint32_t* __restrict__ cnt, uint64_t* __restrict__ sum, uint64_t* __restrict__ abs) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // [bitmaps | sum | abs | cnt], sized by the launcher
  const bool in_lds = bitmap_words <= kMaxLdsBitmapWords;
  const uint32_t copies = (MODE == kLdsCells && ncells <= kSumSpreadCells) ? kSumCopies : 1;
  const int slots = MODE == kGlobalCells ? 0 : ncells * (int)copies;
  uint64_t* s_sum = reinterpret_cast<uint64_t*>(lds + (in_lds ? (bitmap_words + 3) & ~3 : 0));  // 16-byte aligned
  uint64_t* s_abs = s_sum + slots;
  uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_abs + slots);
  if (in_lds)
    for (int i = threadIdx.x; i < bitmap_words; i += kSumBlock) lds[i] = bitmaps[i];
  for (int i = threadIdx.x; i < slots; i += kSumBlock) {
    s_sum[i] = 0;
    s_abs[i] = 0;
    s_cnt[i] = 0;
  }
  __syncthreads();
  const uint32_t copy = threadIdx.x & (copies - 1);  // this lane's copy
  uint32_t a_cnt = 0;                                // kOneCell: the lane's own sums
  uint64_t a_sum = 0, a_abs = 0;
  const ColumnDesc vcd = cols[gk.vcol];
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int64_t row0[kSumU];
    uint16_t lv[kSumU];
#pragma unroll
    for (int u = 0; u < kSumU; ++u) {
      row0[u] = tile * kTileRows + (int64_t)u * (kSumBlock * kRowsPerLane) + (int64_t)threadIdx.x * kRowsPerLane;
      lv[u] = live[row0[u] >> 4];
    }
    uint32_t m[kSumU];
    if (in_lds) run_program<kSumU>(cols, prog, prog_len, (const uint32_t*)lds, row0, m);
    else run_program<kSumU>(cols, prog, prog_len, bitmaps, row0, m);
#pragma unroll
    for (int u = 0; u < kSumU; ++u) {
      uint32_t sel = row0[u] < nrows ? (m[u] & (uint32_t)lv[u]) : 0u;
      if (!sel) continue;
      int32_t val[16];
      load16(vcd, row0[u], val);
      int64_t num[16];  // the 16 gathers in flight together
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const bool ok = ((sel >> i) & 1u) && (uint32_t)val[i] < nvalues;  // -1 (missing) is past any size
        num[i] = ok ? nums[(uint32_t)val[i]] : kNoNumber;
      }
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (num[i] == kNoNumber) sel &= ~(1u << i);  // unselected, undefined or no number: adds nothing
      if constexpr (MODE == kOneCell) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if (!((sel >> i) & 1u)) continue;
          a_cnt += 1;
          a_sum += (uint64_t)num[i];
          a_abs += (uint64_t)(num[i] < 0 ? -num[i] : num[i]);
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
          const uint64_t s = (uint64_t)num[i], a = (uint64_t)(num[i] < 0 ? -num[i] : num[i]);
          if constexpr (MODE == kLdsCells) merge<true>(s_cnt, s_sum, s_abs, cell[i] * copies + copy, 1u, s, a);
          else merge<false>(cnt, sum, abs, cell[i], 1u, s, a);
        }
      }
    }
  }
  if constexpr (MODE == kOneCell) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      a_cnt += (uint32_t)__shfl_xor((int)a_cnt, off, 64);
      a_sum += shfl_xor64(a_sum, off);
      a_abs += shfl_xor64(a_abs, off);
    }
    if ((threadIdx.x & 63) == 0 && a_cnt) merge<true>(s_cnt, s_sum, s_abs, 0u, a_cnt, a_sum, a_abs);
  }
  if constexpr (MODE != kGlobalCells) {
    __syncthreads();
    for (int i = threadIdx.x; i < ncells; i += kSumBlock) {
      uint32_t n = 0;
      uint64_t s = 0, a = 0;
      for (uint32_t c = 0; c < copies; ++c) {
        const uint32_t k = i * copies + c;
        n += s_cnt[k];
        s += s_sum[k];
        a += s_abs[k];
      }
      if (n) merge<false>(cnt, sum, abs, (uint32_t)i, n, s, a);
    }
  }
}

namespace {
template <int MODE>
int launch_sums(int64_t blocks, size_t lds, hipStream_t stream, const void* cols, int64_t nrows, int64_t tiles,
                const uint16_t* live, const int32_t* prog, int32_t prog_len, const uint32_t* bitmaps,
                int32_t bitmap_words, const SumKeys& gk, int32_t ncells, const int64_t* nums, uint32_t nvalues,
                uint32_t* cnt, uint64_t* sum, uint64_t* abs) {
  hipLaunchKernelGGL(tt_scan_sums<MODE>, dim3((unsigned)blocks), dim3(kSumBlock), lds, stream,
                     reinterpret_cast<const ColumnDesc*>(cols), nrows, tiles, live, prog, prog_len, bitmaps,
                     bitmap_words, gk, ncells, nums, nvalues, cnt, sum, abs);
  return (int)hipGetLastError();
}
}  // namespace

// Preconditions (checked by the Python wrapper): as tt_launch_scan_extrema; `value_col` is the row
// of the column table with the key's dictionary ids, `nums` holds `nvalues` int64 (the m of each
// id, INT64_MIN = no number).  `cnt` / `sum` / `abs` hold prod(dims[i] + 1) cells, zeroed.
// nrows <= 2^32: the count of a cell is 32 bits.  `max_blocks`: 0 = as many blocks as stay
// resident (LDS per block against the CU's, at most 8 per CU).
// -2: more cells than tt_group_max_cells().  Nothing is launched on a refusal.
extern "C" int tt_launch_scan_sums(const void* cols, int64_t nrows, const uint16_t* live, const int32_t* prog,
                                   int32_t prog_len, const uint32_t* bitmaps, int32_t bitmap_words,
                                   const int32_t* keys, const int32_t* dims, int32_t nkeys, int32_t value_col,
                                   const int64_t* nums, int64_t nvalues, uint32_t* cnt, uint64_t* sum, uint64_t* abs,
                                   int32_t max_blocks, hipStream_t stream) {
  if (prog_len <= 0 || nrows < 0 || nrows > (int64_t)1 << 32 || bitmap_words <= 0 || nkeys < 0 ||
      nkeys > kSumMaxKeys || value_col < 0 || max_blocks < 0 || nvalues < 0 || nvalues > (int64_t)1 << 31 ||
      (nvalues > 0 && nums == nullptr))
    return -1;
  SumKeys gk = {};
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
  const int mode = nkeys == 0 ? kOneCell : ncells <= kSumMaxLdsCells ? kLdsCells : kGlobalCells;
  const size_t slots = mode == kGlobalCells ? 0
                       : mode == kLdsCells && ncells <= kSumSpreadCells ? (size_t)ncells * kSumCopies
                                                                        : (size_t)ncells;
  const size_t lds = sizeof(uint32_t) * (bitmap_words <= kMaxLdsBitmapWords ? (size_t)((bitmap_words + 3) & ~3) : 0) +
                     kSumCellBytes * slots;
  int64_t blocks = max_blocks;
  if (blocks == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      return -3;
    int per_cu = lds ? (int)(kSumLdsBudget / lds) : 8;
    per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;
    blocks = (int64_t)cus * per_cu;
  }
  if (blocks > tiles) blocks = tiles;
  static bool lds_raised = false;  // bitmaps + cells go past the 64 KiB default limit
  if (mode == kLdsCells && !lds_raised) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(tt_scan_sums<kLdsCells>),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            sizeof(uint32_t) * kMaxLdsBitmapWords + kSumCellBytes * kSumMaxLdsCells) != hipSuccess)
      return -4;
    lds_raised = true;
  }
  if (mode == kOneCell)
    return launch_sums<kOneCell>(blocks, lds, stream, cols, nrows, tiles, live, prog, prog_len, bitmaps, bitmap_words,
                                 gk, (int32_t)ncells, nums, (uint32_t)nvalues, cnt, sum, abs);
  if (mode == kLdsCells)
    return launch_sums<kLdsCells>(blocks, lds, stream, cols, nrows, tiles, live, prog, prog_len, bitmaps,
                                  bitmap_words, gk, (int32_t)ncells, nums, (uint32_t)nvalues, cnt, sum, abs);
  return launch_sums<kGlobalCells>(blocks, lds, stream, cols, nrows, tiles, live, prog, prog_len, bitmaps,
                                   bitmap_words, gk, (int32_t)ncells, nums, (uint32_t)nvalues, cnt, sum, abs);
}
