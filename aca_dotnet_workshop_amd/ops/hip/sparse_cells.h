// Group cells in an open-addressing hash table in HBM instead of a dense array: what
// tt_scan_sparse (group_sparse.hip) and the kHashedCells mode of scan_reduce (scan_reduce.h) share
// (gfx950 / CDNA4, wave64).  A cell space of any size below 2^62 is aggregated in the scan pass,
// the memory follows the cells that occur, and only those travel to the host.
//
// Cell: the rule of group_cells (scan_cells.h) in 64 bits -- axis i has dims[i] + 1 slots, slot
// dims[i] = "path missing", an id outside [0, dims[i]) that is not -1 drops the row.
// Table: `mask + 1` uint64 keys, a power of two, all-ones = empty (set by the host; cells are
// below 2^62, so no cell equals it).  A cell hashes through a 64-bit finaliser (cells are products
// of small ids: identity plus mask would pile them up) and probes linearly: a key equal to the
// cell is its slot; an empty slot is claimed with one 64-bit compare-and-swap (relaxed, agent
// scope), taken if it won or met the same cell; otherwise the next slot.  Keys never change once
// set.  Counts and value words live in arrays of their own indexed by slot and are read only after
// the kernel ends, so the claim of a key and the atomics on its slot need no order between them.
// The probe is bounded at min(slots, kMaxProbes) steps: past it `*status` is set and the row
// dropped -- a full table ends as a flag the host reads (it discards the answer), never as a long
// kernel.  A block reads `status` before each tile (scan_tiles<true>) and stops once it is set.
#pragma once
#include "scan_cells.h"

namespace {
constexpr int kMaxProbes = 1024;             // at load <= 0.5 the longest run of a table of 2^26 slots stays far below
constexpr uint64_t kEmptyKey = ~0ull;
constexpr uint32_t kNoSlot = ~0u;
constexpr int64_t kMaxSparseCells = ((int64_t)1 << 62) - 1;
constexpr int64_t kMaxSparseSlots = (int64_t)1 << 31;

// The cells of rows [row0, row0 + 16) in 64 bits; clears the sel bit of a dropped row.
__device__ __forceinline__ void group_cells64(const ColumnDesc* __restrict__ cols, const GroupKeys& gk, int64_t row0,
                                              uint32_t& sel, uint64_t (&cell)[16]) {
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
      cell[i] = cell[i] * ((uint64_t)n + 1u) + slot;  // wraps only for dropped rows
    }
  }
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // the finaliser of MurmurHash3
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// The slot of `cell`, found or claimed; kNoSlot (and *status set) when the probe bound is reached.
__device__ __forceinline__ uint32_t sparse_slot(uint64_t* __restrict__ keys, uint32_t mask, uint64_t cell,
                                                uint32_t* __restrict__ status) {
  uint32_t s = (uint32_t)mix64(cell) & mask;
  const uint32_t bound = mask < (uint32_t)kMaxProbes ? mask + 1u : (uint32_t)kMaxProbes;
  for (uint32_t p = 0; p < bound; ++p, s = (s + 1u) & mask) {
    const uint64_t k = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == cell) return s;
    if (k != kEmptyKey) continue;
    uint64_t seen = kEmptyKey;
    if (__hip_atomic_compare_exchange_strong(keys + s, &seen, cell, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT) || seen == cell)
      return s;
  }
  __hip_atomic_fetch_or(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return kNoSlot;
}

// pack_keys for a 64-bit cell space.  -1: a bad argument; -2: prod(dims[i] + 1) >= 2^62.
inline int pack_keys64(const int32_t* keys, const int32_t* dims, int32_t nkeys, int max_keys, GroupKeys& gk) {
  if (nkeys < 0 || nkeys > max_keys) return -1;
  gk = {};
  gk.nkeys = nkeys;
  unsigned __int128 ncells = 1;  // three factors of at most 2^31 each
  for (int i = 0; i < nkeys; ++i) {
    if (keys[i] < 0 || dims[i] < 0) return -1;
    gk.col[i] = keys[i];
    gk.dim[i] = dims[i];
    ncells *= (uint64_t)dims[i] + 1u;
  }
  return ncells > (unsigned __int128)kMaxSparseCells ? -2 : 0;
}

// `slots`: a power of two in [2, 2^31].
inline bool sparse_slots_ok(int64_t slots) {
  return slots >= 2 && slots <= kMaxSparseSlots && (slots & (slots - 1)) == 0;
}
}  // namespace
