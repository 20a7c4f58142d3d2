// The histogram of a sparse group space (gfx950 / CDNA4, wave64): the sibling of tt_scan_group
// (group_agg.hip) for key columns whose dense cell space -- the product of their dictionary sizes --
// is past tt_group_max_cells() while the cells that occur are few: GROUP BY two columns of 2,100
// users each is 4.4 M cells and perhaps a few hundred thousand pairs.
//
// tt_scan_sparse: 0 to 3 key columns; the scan front end is scan_cells.h's, the 64-bit cell and
// the hash table sparse_cells.h's.  Per selected, non-dropped row: counts[sparse_slot(cell)] += 1
// (uint32, integer atomics only: the counts do not depend on the order the rows arrive in; which
// slot a cell takes may).  One dominant group sends every lane to one address, so equal cells among
// a lane's 16 rows are merged in registers first: one probe and one add per distinct cell of the
// row group.  The dynamic LDS holds the staged leaf bitmaps only.
#include "sparse_cells.h"

__global__ void __launch_bounds__(kScanBlock)
tt_scan_sparse(const ColumnDesc* __restrict__ cols,
               int64_t nrows, int64_t tiles,
               const uint16_t* __restrict__ live,      // 1 bit per row, row order
               const int32_t* __restrict__ prog, int32_t prog_len,
               const uint32_t* __restrict__ bitmaps, int32_t bitmap_words,
               GroupKeys gk,
               uint64_t* __restrict__ table_keys, uint32_t* __restrict__ counts, uint32_t mask,
               uint32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // [bitmaps], sized by the launcher
  stage_bitmaps(lds, bitmaps, bitmap_words);
  __syncthreads();
  scan_tiles<true>(cols, nrows, tiles, live, prog, prog_len, bitmaps, bitmap_words, lds,
                   [&](int64_t row0, uint32_t sel) __attribute__((always_inline)) {
                     uint64_t cell[16];
                     group_cells64(cols, gk, row0, sel, cell);
#pragma unroll
                     for (int i = 0; i < 16; ++i) {
                       if (!((sel >> i) & 1u)) continue;
                       uint32_t n = 1;
#pragma unroll
                       for (int j = i + 1; j < 16; ++j) {  // the later rows of the same cell ride along
                         const bool same = ((sel >> j) & 1u) && cell[j] == cell[i];
                         n += same;
                         sel &= ~((uint32_t)same << j);
                       }
                       const uint32_t slot = sparse_slot(table_keys, mask, cell[i], status);
                       if (slot != kNoSlot) atomicAdd(&counts[slot], n);
                     }
                   },
                   status);
}

// Preconditions (checked by the Python wrapper): as tt_launch_scan_group.  `table_keys`: `slots`
// uint64 set to all-ones; `counts`: `slots` zeroed uint32; `status`: one zeroed uint32, non-zero
// afterwards when a probe reached its bound (the table is too full: discard the answer).
// -1: a bad argument, `slots` not a power of two in [2, 2^31], nrows > 2^32 (a count is 32 bits),
// more than 3 keys; -2: prod(dims[i] + 1) >= 2^62.  Nothing is launched on a refusal.
extern "C" int tt_launch_scan_sparse(const void* cols, int64_t nrows, const uint16_t* live, const int32_t* prog,
                                     int32_t prog_len, const uint32_t* bitmaps, int32_t bitmap_words,
                                     const int32_t* keys, const int32_t* dims, int32_t nkeys, uint64_t* table_keys,
                                     uint32_t* counts, int64_t slots, uint32_t* status, int32_t max_blocks,
                                     hipStream_t stream) {
  if (prog_len <= 0 || nrows < 0 || nrows > (int64_t)1 << 32 || bitmap_words <= 0 || max_blocks < 0 ||
      !sparse_slots_ok(slots) || !table_keys || !counts || !status)
    return -1;
  GroupKeys gk;
  if (const int rc = pack_keys64(keys, dims, nkeys, kMaxGroupKeys, gk)) return rc;
  const int64_t tiles = (nrows + kTileRows - 1) / kTileRows;
  if (tiles == 0) return 0;
  const size_t lds = bitmap_lds_bytes(bitmap_words);
  const int64_t blocks = resident_blocks(max_blocks, lds, tiles);
  if (blocks < 0) return (int)blocks;
  hipLaunchKernelGGL(tt_scan_sparse, dim3((unsigned)blocks), dim3(kScanBlock), lds, stream,
                     reinterpret_cast<const ColumnDesc*>(cols), nrows, tiles, live, prog, prog_len, bitmaps,
                     bitmap_words, gk, table_keys, counts, (uint32_t)(slots - 1), status);
  return (int)hipGetLastError();
}

extern "C" int tt_sparse_max_probes() { return kMaxProbes; }
