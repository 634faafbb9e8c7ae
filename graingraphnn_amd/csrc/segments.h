// Disjoint unions: the nodes of n segments -- trajectories, frames, images, samples of a batch -- lie one segment
// after the other, and a rising int64 off[n + 1] holds every segment's first node: segment s owns [off[s], off[s + 1]), equal
// offsets are an empty segment.  The one rule "which segment holds node v", for every stage that takes such a union.
// Indices are int: every entry point whose n gets here bounds it by SEG_MAX or less (seg_union_ok below,
// GGNN_JUNCTION_MAX_BLOCKS, GGNN_COLLATE_MAX_BATCH), so no caller needs a wider search and the helper is no template.
#pragma once
#include <stdint.h>

namespace ggnn {

constexpr int64_t SEG_MAX = 1 << 29;   // the most segments an entry point accepts

// The last s in [0, n) with off[s] <= v, or 0 when there is none: a node on an offset belongs to the segment that begins there,
// empty segments are stepped over, n = 1 reads nothing.  off[0] and off[n] are not read; `off` is global memory or LDS.
__device__ __forceinline__ int seg_of(const int64_t* __restrict__ off, int n, int64_t v) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= v) lo = mid;
    else hi = mid;
  }
  return lo;
}

// v's index inside its segment.
__device__ __forceinline__ int64_t seg_local(const int64_t* __restrict__ off, int n, int64_t v) { return v - off[seg_of(off, n, v)]; }

// Is v the first node of a segment that has nodes?  Without offsets the union is its one segment: node 0.  A v at or beyond
// off[n] is nobody's first node, also where empty segments end the union.
__device__ __forceinline__ bool seg_is_first(const int64_t* __restrict__ off, int n, int64_t v) {
  if (off == nullptr) return v == 0;
  return v < off[n] && off[seg_of(off, n, v)] == v;
}

// The union arguments of an entry point: [n + 1] offsets at `off`.  null_is_one: a NULL `off` is the one-segment case and n must
// be 1; otherwise NULL is refused.
static inline bool seg_union_ok(const int64_t* off, int64_t n, bool null_is_one) {
  return off ? n >= 1 && n <= SEG_MAX : null_is_one && n == 1;
}

}  // namespace ggnn
