// MIN / MAX / COUNT(key) per group in the scan pass (gfx950 / CDNA4, wave64): the sibling of
// tt_scan_group (group_agg.hip) for aggregate keys with too many distinct values for a histogram
// -- timestamps, one new dictionary value per write.  Three numbers per group instead of one
// counter per (group, value).
//
// tt_scan_extrema: scan_reduce (scan_reduce.h: the scan front end and the group cell of
// tt_scan_group, 0 to 2 group columns, the three instantiations kOneCell / kLdsCells /
// kGlobalCells) with the policy below.
// One value column: a row of the column table whose codes order as the values do (a rank-encoded
// copy, tt_rank_encode) and are compared as unsigned 32-bit integers; the all-ones code of its
// width (-1 after load16) = undefined.  For every selected, non-dropped row with a defined value:
//   counts[cell] += 1;  lo[cell] = min(lo[cell], code << 32 | row);  hi[cell] = max(hi[cell], same)
// The caller initialises counts = 0, lo = all-ones, hi = 0; lo / hi of a cell mean something only
// where counts > 0.  The row under the code lets the host turn an extremum back into a value with
// one ids[col, row] lookup per group; ties on the code go to the lowest / highest row.
// Most rows do not improve an extremum: the current lo / hi is read first (one untorn 64-bit
// load) and the atomic skipped when the row cannot win.  lo only falls and hi only rises, so a
// stale read costs a redundant atomic, never a wrong result.
#include "scan_reduce.h"

namespace {
struct Extrema {
  using Value = int32_t;  // the code; its word is code << 32 | row
  struct Args {};
  static constexpr uint64_t kIdA = ~0ull, kIdB = 0;

  static __device__ __forceinline__ void load(const ColumnDesc& vcd, const Args&, int64_t row0, uint32_t& sel,
                                              Value (&code)[16]) {
    load16(vcd, row0, code);
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (code[i] == -1) sel &= ~(1u << i);  // undefined: counts nowhere
  }
  static __device__ __forceinline__ uint64_t word_a(Value code, int64_t row) {  // row < 2^32 (launcher)
    return ((uint64_t)(uint32_t)code << 32) | (uint64_t)row;
  }
  static __device__ __forceinline__ uint64_t word_b(Value code, int64_t row) { return word_a(code, row); }
  static __device__ __forceinline__ uint64_t join_a(uint64_t x, uint64_t y) { return y < x ? y : x; }
  static __device__ __forceinline__ uint64_t join_b(uint64_t x, uint64_t y) { return y > x ? y : x; }

  // n rows with keys in [klo, khi] into slot idx.
  template <bool LDS>
  static __device__ __forceinline__ void merge(uint32_t* cnt, uint64_t* lo, uint64_t* hi, uint32_t idx, uint32_t n,
                                               uint64_t klo, uint64_t khi) {
    constexpr int scope = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
    __hip_atomic_fetch_add(cnt + idx, n, __ATOMIC_RELAXED, scope);
    if (klo < __hip_atomic_load(lo + idx, __ATOMIC_RELAXED, scope))
      __hip_atomic_fetch_min(lo + idx, klo, __ATOMIC_RELAXED, scope);
    if (khi > __hip_atomic_load(hi + idx, __ATOMIC_RELAXED, scope))
      __hip_atomic_fetch_max(hi + idx, khi, __ATOMIC_RELAXED, scope);
  }
};
}  // namespace

// kOneCell and kGlobalCells are held to 4 waves per SIMD, as many as their registers allowed while
// the scan loop and the cell rule were written out in the kernel (110 and 116 VGPRs; the 80 and 88
// they take now would admit 6 and 5).  More waves run more blocks at a time, and that measured
// slower (profiles/group_extrema.md): kGlobalCells over a key that rises with the row (a timestamp
// written in order), where more rows then find themselves the new maximum of their group and pay
// the atomic -- 1.70 ms against 1.56 ms at 1e8 rows, 30 % selected, 100,000 groups; kOneCell by
// 3 % with 30 % and 100 % selected.  kLdsCells gained from its fifth and sixth wave and keeps them.
template <int MODE>
__global__ void __launch_bounds__(kScanBlock) __attribute__((amdgpu_waves_per_eu(1, MODE == kLdsCells ? 8 : 4)))
tt_scan_extrema(const ColumnDesc* __restrict__ cols,
                int64_t nrows, int64_t tiles,
                const uint16_t* __restrict__ live,      // 1 bit per row, row order
                const int32_t* __restrict__ prog, int32_t prog_len,
                const uint32_t* __restrict__ bitmaps, int32_t bitmap_words,
                GroupKeys gk, int32_t ncells,
                uint32_t* __restrict__ counts, uint64_t* __restrict__ lo, uint64_t* __restrict__ hi) {
  scan_reduce<Extrema, MODE>(cols, nrows, tiles, live, prog, prog_len, bitmaps, bitmap_words, gk, ncells, {}, counts,
                             lo, hi);
}

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
  ReducePlan p;
  if (const int rc = plan_reduce(nrows, prog_len, bitmap_words, keys, dims, nkeys, value_col, max_blocks, p);
      rc || !p.tiles)
    return rc;
  const auto kernel = p.mode == kOneCell    ? tt_scan_extrema<kOneCell>
                      : p.mode == kLdsCells ? tt_scan_extrema<kLdsCells>
                                            : tt_scan_extrema<kGlobalCells>;
  static bool lds_raised = false;  // bitmaps + cells go past the 64 KiB default limit
  if (p.mode == kLdsCells)
    if (const int rc = raise_dynamic_lds(reinterpret_cast<const void*>(kernel), kMaxReduceLds, lds_raised)) return rc;
  hipLaunchKernelGGL(kernel, dim3((unsigned)p.blocks), dim3(kScanBlock), p.lds, stream,
                     reinterpret_cast<const ColumnDesc*>(cols), nrows, p.tiles, live, prog, prog_len, bitmaps,
                     bitmap_words, p.gk, p.ncells, counts, lo, hi);
  return (int)hipGetLastError();
}

extern "C" int tt_extrema_max_lds_cells() { return kMaxLdsCells; }

// The same reduction over a sparse group space: the cells in a hash table (kHashedCells of
// scan_reduce.h, sparse_cells.h), counts / lo / hi indexed by slot.
__global__ void __launch_bounds__(kScanBlock)
tt_scan_extrema_sparse(const ColumnDesc* __restrict__ cols,
                       int64_t nrows, int64_t tiles,
                       const uint16_t* __restrict__ live,      // 1 bit per row, row order
                       const int32_t* __restrict__ prog, int32_t prog_len,
                       const uint32_t* __restrict__ bitmaps, int32_t bitmap_words,
                       GroupKeys gk,
                       uint32_t* __restrict__ counts, uint64_t* __restrict__ lo, uint64_t* __restrict__ hi,
                       uint64_t* __restrict__ table_keys, uint32_t mask, uint32_t* __restrict__ status) {
  scan_reduce<Extrema, kHashedCells>(cols, nrows, tiles, live, prog, prog_len, bitmaps, bitmap_words, gk, 0, {},
                                     counts, lo, hi, table_keys, mask, status);
}

// As tt_launch_scan_extrema, for any cell space below 2^62 (-2 at or past it).  `table_keys`:
// `slots` uint64 set to all-ones, `slots` a power of two in [2, 2^31]; `counts` / `lo` / `hi` hold
// `slots` elements initialised to 0 / all-ones / 0 and are indexed by slot; `status`: one zeroed
// uint32, non-zero afterwards when the table was too full (discard the answer).
extern "C" int tt_launch_scan_extrema_sparse(const void* cols, int64_t nrows, const uint16_t* live,
                                             const int32_t* prog, int32_t prog_len, const uint32_t* bitmaps,
                                             int32_t bitmap_words, const int32_t* keys, const int32_t* dims,
                                             int32_t nkeys, int32_t value_col, uint32_t* counts, uint64_t* lo,
                                             uint64_t* hi, uint64_t* table_keys, int64_t slots, uint32_t* status,
                                             int32_t max_blocks, hipStream_t stream) {
  if (!counts || !lo || !hi || !table_keys || !status) return -1;
  ReducePlan p;
  if (const int rc = plan_reduce_sparse(nrows, prog_len, bitmap_words, keys, dims, nkeys, value_col, slots,
                                        max_blocks, p);
      rc || !p.tiles)
    return rc;
  hipLaunchKernelGGL(tt_scan_extrema_sparse, dim3((unsigned)p.blocks), dim3(kScanBlock), p.lds, stream,
                     reinterpret_cast<const ColumnDesc*>(cols), nrows, p.tiles, live, prog, prog_len, bitmaps,
                     bitmap_words, p.gk, counts, lo, hi, table_keys, (uint32_t)(slots - 1), status);
  return (int)hipGetLastError();
}
