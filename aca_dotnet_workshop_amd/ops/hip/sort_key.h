// The packed ordering key of sort_keys.hip and page_topk.hip, most significant first:
//     [rank(key0) | rank(key1) | ... | seq]
// rank(k) is the value's position in the column dictionary's sort order (a missing path ranks
// like null; a DESC key stores max_rank - rank), seq the document's insertion sequence.  The
// host's definition of the same key is ops/columnar.py (sort_fields, sort_keys_numpy).
#pragma once
#include "scan_common.h"

namespace {

constexpr int kMaxSortKeys = 4;

struct SortSpec {     // host-built, one per sort key (primary first)
  int32_t col;        // column index into the column table
  int32_t rank_off;   // offset of this key's rank table in `ranks`
  int32_t nranks;     // entries in this key's rank table (dictionary size)
  int32_t bits;       // key field width
  int32_t desc;       // 1 = descending
  int32_t missing;    // rank of a missing path
  int32_t max_rank;   // for DESC: stored value = max_rank - rank
  int32_t pad;
};

// Append one sort key's field (rank `r` of the row's value) to the key built so far.
__device__ __forceinline__ uint64_t pack_rank(uint64_t k, const SortSpec& s, int32_t r) {
  return (k << s.bits) | (uint64_t)(uint32_t)(s.desc ? s.max_rank - r : r);
}

// The key's tail: the insertion sequence breaks ties (and makes every key unique).
__device__ __forceinline__ uint64_t pack_seq(uint64_t k, int seq_bits, uint32_t seq) {
  return (k << seq_bits) | (uint64_t)seq;
}

}  // namespace
