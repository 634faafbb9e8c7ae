// Training targets from a recorded sequence of grain-ID images: the frames are the images of ONE union
// (ggnn_image_junctions_traj / ggnn_junction_links_traj, vectorize.hip), every frame holding the same grains under the same
// ids, and what the reference's junction tracker (graph_trajectory.py:283-846) and form_gradient (graph_datastruct.py:851-1011)
// derive from its solver's output is derived here from the union's own arrays, on the device:
//   ggnn_track_junctions = per junction, the junction of the next and of the previous frame with the same grain triple
//   ggnn_track_targets   = node targets, masks, grain events, edge labels, history columns and the per-pair counters
// The rule is exact in integers up to the fp64 expressions of the targets, which are rounded to fp32 once (include/ggnn.h;
// tests/trackcheck.py restates it).  A junction's partner holds the junction's grains, shifted to the other frame, so it lies
// in the joint->grain row of the shifted first grain: a thread per junction walks that row -- about six junctions -- and
// compares triples.  No sort, no hash, no LDS; nothing is ordered by an atomic (the counters are sums).
// Every index is clamped as in vectorize.hip: rows to [0, E_cap], columns to [0, n_joint), grain offsets to [0, n_grain],
// nothing is read or written at or beyond joint_capacity; indices into the union are 64-bit.
#include "common.h"
#include "segments.h"

namespace ggnn {

namespace {

constexpr int TRK_BLOCK = 256;

struct TrackTables {
  const int32_t* __restrict__ triples;
  const int32_t* __restrict__ rowptr;
  const int32_t* __restrict__ col;
  const int64_t* __restrict__ grain_off;
  const int64_t* __restrict__ status;
  int64_t n_grain, n_joint, E_cap, n_frame;
  int32_t boundary;
};

// The grains of frame t: -> the first one, n = how many (0 when the offsets do not rise).
__device__ __forceinline__ int64_t frame_grains(const TrackTables& T, int64_t t, int64_t& n) {
  const int64_t lo = min(max(T.grain_off[t], (int64_t)0), T.n_grain), hi = min(max(T.grain_off[t + 1], lo), T.n_grain);
  n = hi - lo;
  return lo;
}

// status_is_valid of frame t, from its status row: nothing dropped and Euler's formula for the boundary.
__device__ __forceinline__ bool frame_valid(const TrackTables& T, int64_t t) {
  if (t < 0 || t >= T.n_frame) return false;
  const int64_t* s = T.status + t * GGNN_JUNCTION_STATUS_WORDS;
  return s[6] == 0 && s[3] == 0 && s[4] == 0 && s[0] == 2 * s[5] - (T.boundary == GGNN_BC_NOFLUX ? 2 : 0);
}

// The pair (t, t + 1) is emitted: both frames exist and are valid.
__device__ __forceinline__ bool pair_valid(const TrackTables& T, int64_t t) { return frame_valid(T, t) && frame_valid(T, t + 1); }

__device__ __forceinline__ void sort3(int64_t& a, int64_t& b, int64_t& c) {
  const int64_t lo = min(a, min(b, c)), hi = max(a, max(b, c));
  b = a ^ b ^ c ^ lo ^ hi;   // (the middle one: the other two cancel)
  a = lo, c = hi;
}

// How many junctions carry the sorted triple (a, b, c) of union grains, and the last of them: the row of a.
__device__ __forceinline__ int find_triple(const TrackTables& T, int64_t a, int64_t b, int64_t c, int64_t& at) {
  int found = 0;
  at = -1;
  if (a < 0 || a >= T.n_grain) return 0;
  const int64_t p0 = min((int64_t)max(T.rowptr[a], 0), T.E_cap);
  const int64_t p1 = min(max((int64_t)T.rowptr[a + 1], p0), T.E_cap);
  for (int64_t p = p0; p < p1; ++p) {
    const int64_t o = T.col[p];
    if (o < 0 || o >= T.n_joint) continue;
    if (T.triples[3 * o] == a && T.triples[3 * o + 1] == b && T.triples[3 * o + 2] == c) ++found, at = o;
  }
  return found;
}

// The sorted triple (a, b, c) of frame `from`, as the grains of frame `to`: false when `to` has no such grains.
__device__ __forceinline__ bool shift_triple(const TrackTables& T, int64_t from, int64_t to, int64_t& a, int64_t& b, int64_t& c) {
  int64_t n_from, n_to;
  const int64_t g_from = frame_grains(T, from, n_from), g_to = frame_grains(T, to, n_to);
  const int64_t la = a - g_from, lb = b - g_from, lc = c - g_from;
  if (la < 0 || lc >= n_to) return false;
  a = g_to + la, b = g_to + lb, c = g_to + lc;
  return true;
}

// v summed over the lanes for which `live` holds and added to counter[t]: one atomic a wave where the wave's live lanes stand in
// one frame (nearly always: a frame holds hundreds of junctions), one a lane otherwise.  Every lane of the wave calls this.
__device__ __forceinline__ void count_add(int64_t* __restrict__ counters, int words, int word, int64_t t, bool live,
                                          unsigned long long v) {
  const unsigned long long lanes = __ballot(live);
  if (!lanes) return;
  const int first = __ffsll(lanes) - 1;
  const int64_t t0 = (int64_t)__shfl((long long)t, first);
  const bool uniform = __all(!live || t == t0);
  if (uniform) {
    unsigned long long sum = live ? v : 0;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s);
    if ((int)(threadIdx.x & 63) == first && sum) atomicAdd((unsigned long long*)counters + t0 * words + word, sum);
  } else if (live && v) {
    atomicAdd((unsigned long long*)counters + t * words + word, v);
  }
}

__device__ __forceinline__ TrackTables tables(const int32_t* triples, const int32_t* rowptr, const int32_t* col,
                                              const int64_t* grain_off, const int64_t* status, int64_t n_grain,
                                              int64_t joint_capacity, int64_t E_cap, int64_t n_frame, int32_t boundary) {
  TrackTables T;
  T.triples = triples, T.rowptr = rowptr, T.col = col, T.grain_off = grain_off, T.status = status;
  T.n_grain = n_grain, T.E_cap = E_cap, T.n_frame = n_frame, T.boundary = boundary;
  T.n_joint = min(max(status[n_frame * GGNN_JUNCTION_STATUS_WORDS + n_frame], (int64_t)0), joint_capacity);
  return T;
}

// One thread a junction: its triple counted in its own frame, in the next and in the previous one.
__global__ __launch_bounds__(TRK_BLOCK) void track_junctions_kernel(const ggnn_track_args A) {
  const TrackTables T = tables(A.triples, A.rowptr, A.col, A.grain_off, A.status, A.n_grain, A.joint_capacity, A.E_cap,
                               A.n_frame, A.boundary);
  const int64_t* joint_off = A.status + A.n_frame * GGNN_JUNCTION_STATUS_WORDS;
  const int64_t j = (int64_t)blockIdx.x * TRK_BLOCK + threadIdx.x;
  const bool live = j < T.n_joint;
  int64_t t = 0;
  bool matched = false, ambiguous = false;
  if (live) {
    t = seg_of(joint_off, (int)A.n_frame, j);
    const int64_t a = T.triples[3 * j], b = T.triples[3 * j + 1], c = T.triples[3 * j + 2];
    int64_t at;
    const int own = find_triple(T, a, b, c, at);
    int64_t next = -1, prev = -1;
    if (pair_valid(T, t)) {
      int64_t sa = a, sb = b, sc = c;
      const int there = shift_triple(T, t, t + 1, sa, sb, sc) ? find_triple(T, sa, sb, sc, at) : 0;
      if (own == 1 && there == 1) next = at;
      matched = next >= 0;
      ambiguous = own > 1 || there > 1;
    }
    if (pair_valid(T, t - 1)) {
      int64_t sa = a, sb = b, sc = c;
      const int there = shift_triple(T, t, t - 1, sa, sb, sc) ? find_triple(T, sa, sb, sc, at) : 0;
      if (own == 1 && there == 1) prev = at;
    }
    A.next_joint[j] = next;
    A.prev_joint[j] = prev;
  }
  count_add(A.counters, 2, 0, t, live, matched ? 1 : 0);
  count_add(A.counters, 2, 1, t, live, ambiguous ? 1 : 0);
}

// 5 (to - from) of one coordinate, formed in fp64 and rounded once; periodic: the minimum image (periodGATconv.py:209-210).
__device__ __forceinline__ float joint_step(float from, float to, bool periodic) {
  double d = (double)to - (double)from;
  if (periodic) d = d > 0.5 ? d - 1.0 : d < -0.5 ? d + 1.0 : d;
  return (float)(5.0 * d);
}

// Junction p is the destination of one of junction o's three joint->joint columns.
__device__ __forceinline__ bool linked(const int64_t* __restrict__ jj_dst, int64_t o, int64_t p) {
  return jj_dst[3 * o] == p || jj_dst[3 * o + 1] == p || jj_dst[3 * o + 2] == p;
}

// One thread a joint->joint column s = 3 j + k of the union: its label; the thread of k == 0 also writes junction j's rows.
__global__ __launch_bounds__(TRK_BLOCK) void track_joint_targets_kernel(const ggnn_track_targets_args A) {
  const TrackTables T = tables(A.triples, A.rowptr, A.col, A.grain_off, A.status, A.n_grain, A.joint_capacity, A.E_cap,
                               A.n_frame, A.boundary);
  const int64_t* joint_off = A.status + A.n_frame * GGNN_JUNCTION_STATUS_WORDS;
  const int64_t* jj_dst = A.edge_jj + 3 * A.joint_capacity;
  const int64_t s = (int64_t)blockIdx.x * TRK_BLOCK + threadIdx.x;
  const bool periodic = A.boundary == GGNN_BC_PERIODIC;
  bool live = s < 3 * T.n_joint;
  int64_t t = 0, label = -1;
  if (live) {
    const int64_t j = s / 3;
    const int k = (int)(s - 3 * j);
    t = seg_of(joint_off, (int)A.n_frame, j);
    const int64_t nu = A.next_joint[j];
    if (k == 0) {
      const int64_t pu = A.prev_joint[j];
      const bool fwd = nu >= 0 && nu < T.n_joint, back = pu >= 0 && pu < T.n_joint;
      for (int c = 0; c < 2; ++c) {
        A.y_joint[2 * j + c] = fwd ? joint_step(A.xy[2 * j + c], A.xy[2 * nu + c], periodic) : 0.0f;
        A.hist_joint[2 * j + c] = back ? joint_step(A.xy[2 * pu + c], A.xy[2 * j + c], periodic) : 0.0f;
      }
      A.mask_joint[j] = fwd ? 1.0f : 0.0f;
    }
    live = pair_valid(T, t);   // (the columns of a frame without an emitted pair stay unlabelled and are not counted)
    const int64_t v = jj_dst[s];
    if (live && v >= 0 && v < T.n_joint && v != j) {
      const int64_t nv = A.next_joint[v];
      if (nu >= 0 && nu < T.n_joint && nv >= 0 && nv < T.n_joint) {
        label = linked(jj_dst, nu, nv) ? 0 : -1;
      } else if (nu < 0 && nv < 0) {
        // a neighbour switch: u = {a, b, c}, v = {a, b, d} become {a, c, d} and {b, c, d}, linked through (c, d)
        const int64_t a = T.triples[3 * j + (k == 2 ? 1 : 0)], b = T.triples[3 * j + (k == 0 ? 1 : 2)], c = T.triples[3 * j + 2 - k];
        int64_t d = -1;
        int others = 0;
        for (int i = 0; i < 3; ++i) {
          const int64_t g = T.triples[3 * v + i];
          if (g != a && g != b) d = g, ++others;
        }
        if (others == 1 && d != c) {
          int64_t p0 = a, p1 = c, p2 = d, q0 = b, q1 = c, q2 = d, p = -1, q = -1;
          sort3(p0, p1, p2);
          sort3(q0, q1, q2);
          if (shift_triple(T, t, t + 1, p0, p1, p2) && shift_triple(T, t, t + 1, q0, q1, q2) &&
              find_triple(T, p0, p1, p2, p) == 1 && find_triple(T, q0, q1, q2, q) == 1 && linked(jj_dst, p, q))
            label = 1;
        }
      }
    }
    A.edge_label[s] = live ? label : -1;
  }
  count_add(A.counters, 4, 0, t, live, label == 0 ? 1 : 0);
  count_add(A.counters, 4, 1, t, live, label == 1 ? 1 : 0);
  count_add(A.counters, 4, 2, t, live, label == -1 ? 1 : 0);
}

// 20 (to / pp - from / pp), formed in fp64 and rounded once (form_gradient:868-871).
__device__ __forceinline__ float area_step(uint64_t from, uint64_t to, double pp) {
  return (float)(20.0 * ((double)to / pp - (double)from / pp));
}

// One thread a union grain: its targets towards the next frame and its history from the previous one.
__global__ __launch_bounds__(TRK_BLOCK) void track_grain_targets_kernel(const ggnn_track_targets_args A) {
  const TrackTables T = tables(A.triples, A.rowptr, A.col, A.grain_off, A.status, A.n_grain, A.joint_capacity, A.E_cap,
                               A.n_frame, A.boundary);
  const int64_t g = (int64_t)blockIdx.x * TRK_BLOCK + threadIdx.x;
  const bool live = g < A.n_grain;
  int64_t t = 0;
  bool gone = false;
  if (live) {
    t = seg_of(A.grain_off, (int)A.n_frame, g);
    int64_t n_own, n_next = 0, n_prev = 0;
    const int64_t g0 = frame_grains(T, t, n_own), l = g - g0;
    const bool inside = l >= 0 && l < n_own;   // (false only for offsets that do not cover the union)
    const bool wall = A.boundary == GGNN_BC_NOFLUX && l == 0;
    const uint64_t c = A.pixel_counts[g];
    const int64_t next0 = t + 1 < A.n_frame ? frame_grains(T, t + 1, n_next) : 0;
    const int64_t prev0 = t >= 1 ? frame_grains(T, t - 1, n_prev) : 0;
    const bool fwd = inside && l < n_next && pair_valid(T, t), back = inside && l < n_prev && pair_valid(T, t - 1);
    const uint64_t c_next = fwd ? A.pixel_counts[next0 + l] : 0, c_prev = back ? A.pixel_counts[prev0 + l] : 0;
    const bool present = fwd && c != 0 && !wall;
    gone = present && c_next == 0;
    A.y_grain[2 * g] = fwd ? area_step(c, c_next, A.patch_pixels) : 0.0f;
    A.y_grain[2 * g + 1] = fwd && A.extra_volume ? (float)(20.0 * A.extra_volume[next0 + l]) : 0.0f;
    A.mask_grain[g] = present ? 1.0f : 0.0f;
    A.grain_event[g] = gone ? 1 : 0;
    const bool here = inside && c != 0 && !wall;   // (the row of an absent grain keeps no history)
    A.hist_grain[2 * g] = back && here ? area_step(c_prev, c, A.patch_pixels) : 0.0f;
    A.hist_grain[2 * g + 1] = here && A.extra_volume ? (float)(20.0 * A.extra_volume[g]) : 0.0f;
  }
  count_add(A.counters, 4, 3, t, live, gone ? 1 : 0);
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

}  // namespace ggnn

extern "C" int ggnn_track_junctions(const ggnn_track_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_track_args& A = *args;
  if (!A.triples || !A.rowptr || !A.col || !A.grain_off || !A.status || !A.next_joint || !A.prev_joint || !A.counters)
    return GGNN_EINVAL;
  if (A.n_grain < 1 || A.n_grain >= INT32_MAX - 1 || A.E_cap < 0 || A.E_cap >= INT32_MAX) return GGNN_EINVAL;
  if (A.joint_capacity < 1 || A.joint_capacity > INT32_MAX / 3) return GGNN_EINVAL;
  if (A.n_frame < 2 || A.n_frame > GGNN_JUNCTION_MAX_BLOCKS) return GGNN_EINVAL;
  if (A.boundary != GGNN_BC_PERIODIC && A.boundary != GGNN_BC_NOFLUX) return GGNN_EINVAL;
  if (!aligned8(A.grain_off) || !aligned8(A.status) || !aligned8(A.next_joint) || !aligned8(A.prev_joint) || !aligned8(A.counters))
    return GGNN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(A.counters, 0, (size_t)A.n_frame * 2 * sizeof(int64_t), st) != hipSuccess) return GGNN_ELAUNCH;
  const int64_t blocks = (A.joint_capacity + TRK_BLOCK - 1) / TRK_BLOCK;
  hipLaunchKernelGGL(track_junctions_kernel, dim3((unsigned)blocks), dim3(TRK_BLOCK), 0, st, A);
  return launch_status();
}

extern "C" int ggnn_track_targets(const ggnn_track_targets_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_track_targets_args& A = *args;
  if (!A.triples || !A.rowptr || !A.col || !A.edge_jj || !A.xy || !A.pixel_counts || !A.grain_off || !A.status ||
      !A.next_joint || !A.prev_joint || !A.y_joint || !A.mask_joint || !A.hist_joint || !A.edge_label || !A.y_grain ||
      !A.mask_grain || !A.grain_event || !A.hist_grain || !A.counters)
    return GGNN_EINVAL;
  if (A.n_grain < 1 || A.n_grain >= INT32_MAX - 1 || A.E_cap < 0 || A.E_cap >= INT32_MAX) return GGNN_EINVAL;
  if (A.joint_capacity < 1 || A.joint_capacity > INT32_MAX / 3) return GGNN_EINVAL;
  if (A.n_frame < 2 || A.n_frame > GGNN_JUNCTION_MAX_BLOCKS) return GGNN_EINVAL;
  if (A.boundary != GGNN_BC_PERIODIC && A.boundary != GGNN_BC_NOFLUX) return GGNN_EINVAL;
  if (!(A.patch_pixels >= 1.0)) return GGNN_EINVAL;
  if (!aligned8(A.edge_jj) || !aligned8(A.pixel_counts) || !aligned8(A.extra_volume) || !aligned8(A.grain_off) ||
      !aligned8(A.status) || !aligned8(A.next_joint) || !aligned8(A.prev_joint) || !aligned8(A.edge_label) ||
      !aligned8(A.grain_event) || !aligned8(A.counters))
    return GGNN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(A.counters, 0, (size_t)A.n_frame * 4 * sizeof(int64_t), st) != hipSuccess) return GGNN_ELAUNCH;
  const int64_t joint_blocks = (3 * A.joint_capacity + TRK_BLOCK - 1) / TRK_BLOCK;
  const int64_t grain_blocks = (A.n_grain + TRK_BLOCK - 1) / TRK_BLOCK;
  hipLaunchKernelGGL(track_joint_targets_kernel, dim3((unsigned)joint_blocks), dim3(TRK_BLOCK), 0, st, A);
  hipLaunchKernelGGL(track_grain_targets_kernel, dim3((unsigned)grain_blocks), dim3(TRK_BLOCK), 0, st, A);
  return launch_status();
}
