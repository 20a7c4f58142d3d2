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
// tt_scan_sums: scan_reduce (scan_reduce.h: the scan front end, the group cell, 0 to 2 group
// columns and the three instantiations kOneCell / kLdsCells / kGlobalCells of the sibling) with the
// policy below.  The value column is the key's own id column (any width); a row whose id is
// missing, at or past `nvalues`, or whose m is INT64_MIN adds nothing.  The caller zeroes cnt /
// sum / abs.  In kGlobalCells the rows add to the output with 64-bit integer atomics.
#include "scan_reduce.h"

namespace {
constexpr int64_t kNoNumber = INT64_MIN;

struct Sums {
  using Value = int64_t;  // m
  struct Args {
    const int64_t* __restrict__ nums;  // id -> m
    uint32_t nvalues;
  };
  static constexpr uint64_t kIdA = 0, kIdB = 0;

  static __device__ __forceinline__ void load(const ColumnDesc& vcd, const Args& t, int64_t row0, uint32_t& sel,
                                              Value (&num)[16]) {
    int32_t val[16];
    load16(vcd, row0, val);
#pragma unroll
    for (int i = 0; i < 16; ++i) {  // the 16 gathers in flight together
      const bool ok = ((sel >> i) & 1u) && (uint32_t)val[i] < t.nvalues;  // -1 (missing) is past any size
      num[i] = ok ? t.nums[(uint32_t)val[i]] : kNoNumber;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (num[i] == kNoNumber) sel &= ~(1u << i);  // unselected, undefined or no number: adds nothing
  }
  static __device__ __forceinline__ uint64_t word_a(Value m, int64_t) { return (uint64_t)m; }  // its two's complement word
  static __device__ __forceinline__ uint64_t word_b(Value m, int64_t) { return (uint64_t)(m < 0 ? -m : m); }
  static __device__ __forceinline__ uint64_t join_a(uint64_t x, uint64_t y) { return x + y; }
  static __device__ __forceinline__ uint64_t join_b(uint64_t x, uint64_t y) { return x + y; }

  // n numbers with sum s and sum of magnitudes a into slot idx.
  template <bool LDS>
  static __device__ __forceinline__ void merge(uint32_t* cnt, uint64_t* sum, uint64_t* abs, uint32_t idx, uint32_t n,
                                               uint64_t s, uint64_t a) {
    constexpr int scope = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
    __hip_atomic_fetch_add(cnt + idx, n, __ATOMIC_RELAXED, scope);
    __hip_atomic_fetch_add(sum + idx, s, __ATOMIC_RELAXED, scope);
    __hip_atomic_fetch_add(abs + idx, a, __ATOMIC_RELAXED, scope);
  }
};
}  // namespace

template <int MODE>
__global__ void __launch_bounds__(kScanBlock)
tt_scan_sums(const ColumnDesc* __restrict__ cols,
             int64_t nrows, int64_t tiles,
             const uint16_t* __restrict__ live,      // 1 bit per row, row order
             const int32_t* __restrict__ prog, int32_t prog_len,
             const uint32_t* __restrict__ bitmaps, int32_t bitmap_words,
             GroupKeys gk, int32_t ncells,
             const int64_t* __restrict__ nums, uint32_t nvalues,   // id -> m
             uint32_t* __restrict__ cnt, uint64_t* __restrict__ sum, uint64_t* __restrict__ abs) {
  scan_reduce<Sums, MODE>(cols, nrows, tiles, live, prog, prog_len, bitmaps, bitmap_words, gk, ncells,
                          {nums, nvalues}, cnt, sum, abs);
}

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
  if (nvalues < 0 || nvalues > (int64_t)1 << 31 || (nvalues > 0 && nums == nullptr)) return -1;
  ReducePlan p;
  if (const int rc = plan_reduce(nrows, prog_len, bitmap_words, keys, dims, nkeys, value_col, max_blocks, p);
      rc || !p.tiles)
    return rc;
  const auto kernel = p.mode == kOneCell    ? tt_scan_sums<kOneCell>
                      : p.mode == kLdsCells ? tt_scan_sums<kLdsCells>
                                            : tt_scan_sums<kGlobalCells>;
  static bool lds_raised = false;  // bitmaps + cells go past the 64 KiB default limit
  if (p.mode == kLdsCells)
    if (const int rc = raise_dynamic_lds(reinterpret_cast<const void*>(kernel), kMaxReduceLds, lds_raised)) return rc;
  hipLaunchKernelGGL(kernel, dim3((unsigned)p.blocks), dim3(kScanBlock), p.lds, stream,
                     reinterpret_cast<const ColumnDesc*>(cols), nrows, p.tiles, live, prog, prog_len, bitmaps,
                     bitmap_words, p.gk, p.ncells, nums, (uint32_t)nvalues, cnt, sum, abs);
  return (int)hipGetLastError();
}

// The same sums over a sparse group space: the cells in a hash table (kHashedCells of
// scan_reduce.h, sparse_cells.h), cnt / sum / abs indexed by slot.
__global__ void __launch_bounds__(kScanBlock)
tt_scan_sums_sparse(const ColumnDesc* __restrict__ cols,
                    int64_t nrows, int64_t tiles,
                    const uint16_t* __restrict__ live,      // 1 bit per row, row order
                    const int32_t* __restrict__ prog, int32_t prog_len,
                    const uint32_t* __restrict__ bitmaps, int32_t bitmap_words,
                    GroupKeys gk,
                    const int64_t* __restrict__ nums, uint32_t nvalues,   // id -> m
                    uint32_t* __restrict__ cnt, uint64_t* __restrict__ sum, uint64_t* __restrict__ abs,
                    uint64_t* __restrict__ table_keys, uint32_t mask, uint32_t* __restrict__ status) {
  scan_reduce<Sums, kHashedCells>(cols, nrows, tiles, live, prog, prog_len, bitmaps, bitmap_words, gk, 0,
                                  {nums, nvalues}, cnt, sum, abs, table_keys, mask, status);
}

// As tt_launch_scan_sums, for any cell space below 2^62 (-2 at or past it).  `table_keys`: `slots`
// uint64 set to all-ones, `slots` a power of two in [2, 2^31]; `cnt` / `sum` / `abs` hold `slots`
// zeroed elements and are indexed by slot; `status`: one zeroed uint32, non-zero afterwards when
// the table was too full (discard the answer).
extern "C" int tt_launch_scan_sums_sparse(const void* cols, int64_t nrows, const uint16_t* live, const int32_t* prog,
                                          int32_t prog_len, const uint32_t* bitmaps, int32_t bitmap_words,
                                          const int32_t* keys, const int32_t* dims, int32_t nkeys, int32_t value_col,
                                          const int64_t* nums, int64_t nvalues, uint32_t* cnt, uint64_t* sum,
                                          uint64_t* abs, uint64_t* table_keys, int64_t slots, uint32_t* status,
                                          int32_t max_blocks, hipStream_t stream) {
  if (nvalues < 0 || nvalues > (int64_t)1 << 31 || (nvalues > 0 && nums == nullptr)) return -1;
  if (!cnt || !sum || !abs || !table_keys || !status) return -1;
  ReducePlan p;
  if (const int rc = plan_reduce_sparse(nrows, prog_len, bitmap_words, keys, dims, nkeys, value_col, slots,
                                        max_blocks, p);
      rc || !p.tiles)
    return rc;
  hipLaunchKernelGGL(tt_scan_sums_sparse, dim3((unsigned)p.blocks), dim3(kScanBlock), p.lds, stream,
                     reinterpret_cast<const ColumnDesc*>(cols), nrows, p.tiles, live, prog, prog_len, bitmaps,
                     bitmap_words, p.gk, nums, (uint32_t)nvalues, cnt, sum, abs, table_keys, (uint32_t)(slots - 1),
                     status);
  return (int)hipGetLastError();
}
