// One count and two 64-bit words per group cell, reduced in the scan pass: the body that
// tt_scan_extrema (group_extrema.hip) and tt_scan_sums (group_sums.hip) share, over the front end
// and the cells of scan_cells.h (0 to 2 group columns, one value column).  For every selected,
// non-dropped row whose value the policy `Op` loads:
//   cnt[cell] += 1;  a[cell] = Op::join_a(a[cell], Op::word_a(v, row));  b[cell] likewise
// The caller initialises cnt = 0, a = Op::kIdA, b = Op::kIdB.  Integer atomics only
// (deterministic).  Three instantiations over dense cells, chosen by the launcher (plan_reduce),
// and one over hashed cells for the *_sparse entry points (plan_reduce_sparse):
//   kOneCell   no group column: the lane reduces its rows in registers over all its tiles, the
//              wave reduces across lanes (shuffles), one lane per wave merges into LDS.
//   kLdsCells  up to kMaxLdsCells cells privatised in LDS (8 + 8 + 4 bytes per cell), flushed once
//              per block after its last tile.  Up to kSpreadCells cells (a boolean group) are kept
//              in kCopies interleaved copies, lane l on copy l mod kCopies, as tt_scan_group keeps
//              its few-cell histograms: 64 lanes do not queue on a handful of LDS words.
//   kGlobalCells  above that, up to tt_group_max_cells(): the rows update the output directly.
//   kHashedCells  any cell space below 2^62: the 64-bit cell of a row (group_cells64) finds or
//              claims a slot of the hash table (sparse_slot, sparse_cells.h) after Op::load cleared
//              the rows without a value -- no slot exists with count 0 -- and the row updates cnt /
//              a / b at that slot directly; they hold one element per slot.
// Dynamic LDS: [bitmaps | a | b | cnt], at most 32 + 80 KiB of the CU's 160.
//
// Op, a compile-time policy with only what differs:
//   Value, Args             a row's value; the kernel's arguments beyond the scan's
//   load(vcd, args, row0, sel, v)   the 16 values of a row group; clears sel for rows without one
//   kIdA, kIdB              the identities of the two words
//   word_a(v, row), word_b  the two words of the value of one row
//   join_a(x, y), join_b    two partial results into one, in registers
//   merge<LDS>(cnt, a, b, idx, n, x, y)   n rows with words x, y into slot idx, atomically; LDS:
//                           workgroup scope, the output: agent scope
#pragma once
#include "sparse_cells.h"

extern "C" int tt_group_max_cells();  // group_agg.hip: the cell cap is the histogram's

namespace {
constexpr int kMaxValueKeys = 2;
constexpr int kMaxLdsCells = 4096;          // 20 B each: 80 KiB
constexpr int kCellBytes = 20;
constexpr size_t kMaxReduceLds = sizeof(uint32_t) * kMaxLdsBitmapWords + (size_t)kCellBytes * kMaxLdsCells;

enum CellMode : int { kOneCell = 0, kLdsCells = 1, kGlobalCells = 2, kHashedCells = 3 };

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int mask) {
  return (uint64_t)__shfl_xor((unsigned long long)v, mask, 64);
}

template <typename Op, int MODE>
__device__ __forceinline__ void scan_reduce(const ColumnDesc* __restrict__ cols, int64_t nrows, int64_t tiles,
                                            const uint16_t* __restrict__ live, const int32_t* __restrict__ prog,
                                            int32_t prog_len, const uint32_t* __restrict__ bitmaps,
                                            int32_t bitmap_words, const GroupKeys& gk, int32_t ncells,
                                            const typename Op::Args& args, uint32_t* __restrict__ cnt,
                                            uint64_t* __restrict__ a, uint64_t* __restrict__ b,
                                            uint64_t* __restrict__ table_keys = nullptr, uint32_t mask = 0,
                                            uint32_t* __restrict__ status = nullptr) {  // kHashedCells
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // [bitmaps | a | b | cnt], sized by the launcher
  const uint32_t copies = (MODE == kLdsCells && ncells <= kSpreadCells) ? kCopies : 1;
  const int slots = MODE == kGlobalCells || MODE == kHashedCells ? 0 : ncells * (int)copies;
  uint64_t* s_a = reinterpret_cast<uint64_t*>(stage_bitmaps(lds, bitmaps, bitmap_words));  // 16-byte aligned
  uint64_t* s_b = s_a + slots;
  uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_b + slots);
  for (int i = threadIdx.x; i < slots; i += kScanBlock) {
    s_a[i] = Op::kIdA;
    s_b[i] = Op::kIdB;
    s_cnt[i] = 0;
  }
  __syncthreads();
  const uint32_t copy = threadIdx.x & (copies - 1);  // this lane's copy
  uint32_t r_cnt = 0;                                // kOneCell: the lane's own reduction
  uint64_t r_a = Op::kIdA, r_b = Op::kIdB;
  const ColumnDesc vcd = cols[gk.vcol];
  scan_tiles<MODE == kHashedCells>(cols, nrows, tiles, live, prog, prog_len, bitmaps, bitmap_words, lds,
             [&](int64_t row0, uint32_t sel) __attribute__((always_inline)) {
               typename Op::Value v[16];
               Op::load(vcd, args, row0, sel, v);
               if constexpr (MODE == kOneCell) {
#pragma unroll
                 for (int i = 0; i < 16; ++i) {
                   if (!((sel >> i) & 1u)) continue;
                   r_cnt += 1;
                   r_a = Op::join_a(r_a, Op::word_a(v[i], row0 + i));
                   r_b = Op::join_b(r_b, Op::word_b(v[i], row0 + i));
                 }
               } else if constexpr (MODE == kHashedCells) {
                 if (!sel) return;
                 uint64_t cell[16];
                 group_cells64(cols, gk, row0, sel, cell);
#pragma unroll
                 for (int i = 0; i < 16; ++i) {
                   if (!((sel >> i) & 1u)) continue;
                   const uint32_t slot = sparse_slot(table_keys, mask, cell[i], status);
                   if (slot != kNoSlot)
                     Op::template merge<false>(cnt, a, b, slot, 1u, Op::word_a(v[i], row0 + i),
                                               Op::word_b(v[i], row0 + i));
                 }
               } else {
                 if (!sel) return;
                 uint32_t cell[16];
                 group_cells(cols, gk, row0, sel, cell);
#pragma unroll
                 for (int i = 0; i < 16; ++i) {
                   if (!((sel >> i) & 1u)) continue;
                   const uint64_t x = Op::word_a(v[i], row0 + i), y = Op::word_b(v[i], row0 + i);
                   if constexpr (MODE == kLdsCells)
                     Op::template merge<true>(s_cnt, s_a, s_b, cell[i] * copies + copy, 1u, x, y);
                   else
                     Op::template merge<false>(cnt, a, b, cell[i], 1u, x, y);
                 }
               }
             },
             status);
  if constexpr (MODE == kOneCell) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      r_cnt += (uint32_t)__shfl_xor((int)r_cnt, off, 64);
      r_a = Op::join_a(r_a, shfl_xor64(r_a, off));
      r_b = Op::join_b(r_b, shfl_xor64(r_b, off));
    }
    if ((threadIdx.x & 63) == 0 && r_cnt) Op::template merge<true>(s_cnt, s_a, s_b, 0u, r_cnt, r_a, r_b);
  }
  if constexpr (MODE != kGlobalCells && MODE != kHashedCells) {
    __syncthreads();
    for (int i = threadIdx.x; i < ncells; i += kScanBlock) {
      uint32_t n = 0;
      uint64_t x = Op::kIdA, y = Op::kIdB;
      for (uint32_t c = 0; c < copies; ++c) {
        const uint32_t s = i * copies + c;
        n += s_cnt[s];
        x = Op::join_a(x, s_a[s]);
        y = Op::join_b(y, s_b[s]);
      }
      if (n) Op::template merge<false>(cnt, a, b, (uint32_t)i, n, x, y);
    }
  }
}

struct ReducePlan {
  GroupKeys gk;
  int32_t ncells;
  int mode;
  int64_t tiles, blocks;  // tiles == 0: nothing to launch
  size_t lds;
};

// What both launchers refuse and decide.  nrows <= 2^32: the count of a cell is 32 bits.
// -1: a bad argument; -2: more cells than tt_group_max_cells(); -3: as resident_blocks.
inline int plan_reduce(int64_t nrows, int32_t prog_len, int32_t bitmap_words, const int32_t* keys,
                       const int32_t* dims, int32_t nkeys, int32_t value_col, int32_t max_blocks, ReducePlan& p) {
  if (prog_len <= 0 || nrows < 0 || nrows > (int64_t)1 << 32 || bitmap_words <= 0 || value_col < 0 || max_blocks < 0)
    return -1;
  int64_t ncells;
  if (const int rc = pack_keys(keys, dims, nkeys, kMaxValueKeys, tt_group_max_cells(), p.gk, ncells)) return rc;
  p.gk.vcol = value_col;
  p.ncells = (int32_t)ncells;
  p.tiles = (nrows + kTileRows - 1) / kTileRows;
  if (p.tiles == 0) return 0;
  p.mode = nkeys == 0 ? kOneCell : ncells <= kMaxLdsCells ? kLdsCells : kGlobalCells;
  const size_t slots = p.mode == kGlobalCells ? 0
                       : p.mode == kLdsCells && ncells <= kSpreadCells ? (size_t)ncells * kCopies
                                                                        : (size_t)ncells;
  p.lds = bitmap_lds_bytes(bitmap_words) + kCellBytes * slots;
  p.blocks = resident_blocks(max_blocks, p.lds, p.tiles);
  return p.blocks < 0 ? (int)p.blocks : 0;
}

// plan_reduce for the hashed entry points: `slots` as tt_launch_scan_sparse takes them.
// -1: a bad argument; -2: prod(dims[i] + 1) >= 2^62; -3: as resident_blocks.
inline int plan_reduce_sparse(int64_t nrows, int32_t prog_len, int32_t bitmap_words, const int32_t* keys,
                              const int32_t* dims, int32_t nkeys, int32_t value_col, int64_t slots,
                              int32_t max_blocks, ReducePlan& p) {
  if (prog_len <= 0 || nrows < 0 || nrows > (int64_t)1 << 32 || bitmap_words <= 0 || value_col < 0 ||
      max_blocks < 0 || !sparse_slots_ok(slots))
    return -1;
  if (const int rc = pack_keys64(keys, dims, nkeys, kMaxValueKeys, p.gk)) return rc;
  p.gk.vcol = value_col;
  p.ncells = 0;
  p.mode = kHashedCells;
  p.tiles = (nrows + kTileRows - 1) / kTileRows;
  if (p.tiles == 0) return 0;
  p.lds = bitmap_lds_bytes(bitmap_words);
  p.blocks = resident_blocks(max_blocks, p.lds, p.tiles);
  return p.blocks < 0 ? (int)p.blocks : 0;
}
}  // namespace
