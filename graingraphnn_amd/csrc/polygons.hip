// The grains' junction polygons of a rollout layer, recorded on the device next to the step: what graph.update()
// (graph_datastruct.py:654-721) leaves in `regions`, `region_coors` and `region_center`.
//   ggnn_grain_polygons = one layer, one launch: per grain the junctions of its row of the joint->grain table, unwrapped as
//                         grain_centres_kernel (step.hip) unwraps them, ordered counter-clockwise round their mean by the
//                         key of counterclock() (:100-116), with the mean and the shoelace area of the ordered polygon
// Everything that decides the order -- the unwrapped coordinates, the centre, the key -- is made of fp32 additions,
// subtractions, comparisons and correctly rounded divisions in ONE fixed order, with no multiply-add that the compiler
// could contract: the same inputs give the same order and the same coordinate bits on any grid, through either row path
// below, and in a numpy restatement (tests/polycheck.py).
//
// The key.  counterclock() sorts by the angle of d = v - centre in [0, 2 pi), then by |d|.  The angle itself is never
// needed, only its order, so the key is (quadrant, q, |dx| + |dy|, position in the row) with q = the share of the
// quadrant's trailing axis in |dx| + |dy|: it rises strictly with the angle inside a quadrant, the seam sits where atan2's
// does (dy >= 0, -0.0 included, is angle 0 upward; dy < 0 is below 2 pi), along one ray |dx| + |dy| orders as |d| does, and
// d = 0 comes first as counterclock's (-pi, 0) does.  One division instead of atan2f, whose device and host versions differ
// in the last place.
//
// Rows.  A row of up to 16 junctions is held by a group of 16 lanes, one vertex each: the min-image chain runs as one
// broadcast per vertex (__shfl of width 16: ds_bpermute, no LDS allocation; DPP cannot broadcast from a lane chosen at run
// time on gfx9), the rank of a vertex is the count of smaller keys among the broadcast ones, and every lane scatters its
// vertex to p0 + rank.  A longer row (the no-flux boundary grain) is taken by the whole wave afterwards, lane l owning the
// vertices l, l + 64, ...: every lane walks the row's chain itself (the loads are the same addresses in all lanes), so any
// length is correct and nothing needs scratch.
#include "common.h"

namespace ggnn {

constexpr int POLY_BLOCK = 256;
constexpr int POLY_GROUP = 16;                          // lanes per grain = the longest row of the group path
constexpr int POLY_GRAINS = POLY_BLOCK / POLY_GROUP;    // grains per block

// The key as two unsigned words whose order is the key's: hi = (quadrant + 1, bits of q), lo = (bits of |dx| + |dy|,
// position).  q and the length are non-negative, so their bit patterns order as they do.
struct PolyKey {
  uint64_t hi, lo;
};

__device__ __forceinline__ PolyKey poly_key(float dx, float dy, int at) {
  const float ax = fabsf(dx), ay = fabsf(dy), den = ax + ay;
  const bool none = !(den > 0.0f);   // the centre itself: counterclock's (-pi, 0), in front of every angle
  const bool upper = dy >= 0.0f, side = upper ? dx > 0.0f : dx < 0.0f;
  const uint32_t quad = none ? 0u : (upper ? (side ? 1u : 2u) : (side ? 3u : 4u));
  const float q = none ? 0.0f : (side ? ay : ax) / den;
  return {((uint64_t)quad << 32) | __float_as_uint(q), ((uint64_t)__float_as_uint(den) << 32) | (uint32_t)at};
}

__device__ __forceinline__ bool poly_less(const PolyKey& a, const PolyKey& b) {
  return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo);
}

__device__ __forceinline__ float min_image(float t, float prev) {   // periodic_move, graph_datastruct.py:55-72
  const float rel = t - prev;
  return t + (rel > 0.5f ? -1.0f : (rel < -0.5f ? 1.0f : 0.0f));
}

// A vertex's rank, and the vertex that follows it round the polygon, from the row's vertices seen one at a time.  Selects
// only: hipcc turned a version of this scan with branches and a struct-valued key into code that lost updates of (nx, ny)
// in the no-flux instantiation of the wave's path.
struct PolyScan {
  PolyKey mine, next, first;   // next: the smallest key above mine; first: the smallest key of all
  int rank;
  float nx, ny, fx, fy;        // their d = v - centre
  __device__ __forceinline__ void start(float dx, float dy, int at) {
    mine = poly_key(dx, dy, at);
    next = first = {~0ull, ~0ull};
    rank = 0;
    nx = ny = fx = fy = 0.0f;
  }
  __device__ __forceinline__ void see(float dx, float dy, int at) {
    const PolyKey k = poly_key(dx, dy, at);
    const bool below = poly_less(k, mine), above = poly_less(mine, k);   // (neither: this vertex itself)
    const bool nearer = above && poly_less(k, next), lowest = poly_less(k, first);
    rank += below ? 1 : 0;
    next.hi = nearer ? k.hi : next.hi, next.lo = nearer ? k.lo : next.lo;
    nx = nearer ? dx : nx, ny = nearer ? dy : ny;
    first.hi = lowest ? k.hi : first.hi, first.lo = lowest ? k.lo : first.lo;
    fx = lowest ? dx : fx, fy = lowest ? dy : fy;
  }
  // d of the vertex behind this one in the order (the last one is followed by the first)
  __device__ __forceinline__ void follower(float& x, float& y) const {
    const bool last = (next.hi & next.lo) == ~0ull;
    x = last ? fx : nx;
    y = last ? fy : ny;
  }
};

struct PolyOut {
  int32_t* joint;
  float *xy, *centre, *area;
};

struct PolyIn {
  const int32_t* col;
  const float *x_joint, *offset;
  int64_t ldxj, n_joint;
  float factor;
  // vertex `at` of the table: its junction and the junction's xy in the global frame (test.py:474)
  __device__ __forceinline__ void load(int at, int& j, float& x, float& y) const {
    const int64_t jj = min((int64_t)max(col[at], 0), n_joint - 1);
    j = (int)jj;
    x = x_joint[jj * ldxj];
    y = x_joint[jj * ldxj + 1];
    if (factor > 1.0f) {
      x = (x + (offset ? offset[2 * jj] : 0.0f)) / factor;
      y = (y + (offset ? offset[2 * jj + 1] : 0.0f)) / factor;
    }
  }
};

// Rows of 0 or 1 junction are copied as they are, with area 0 (graph_datastruct.py:683); the centre is the vertex, or 0.
__device__ __forceinline__ void poly_short_row(const PolyIn& I, const PolyOut& O, int64_t g, int p0, int n) {
  float x = 0.0f, y = 0.0f;
  if (n == 1) {
    int j;
    I.load(p0, j, x, y);
    O.joint[p0] = j;
    O.xy[2 * (int64_t)p0] = x;
    O.xy[2 * (int64_t)p0 + 1] = y;
  }
  O.centre[2 * g] = x;
  O.centre[2 * g + 1] = y;
  O.area[g] = 0.0f;
}

// A row of any length by the whole wave (every lane of the wave must call it, with the same arguments).
template <bool PERIODIC>
__device__ void poly_row_wave(const PolyIn& I, const PolyOut& O, int64_t g, int p0, int n, bool reversed, int lane) {
  int j;
  float x, y, px = 0.0f, py = 0.0f, sx = 0.0f, sy = 0.0f, lox = INFINITY, loy = INFINITY;
  for (int i = 0; i < n; ++i) {
    I.load(p0 + i, j, x, y);
    if (PERIODIC && i > 0) x = min_image(x, px), y = min_image(y, py);
    px = x, py = y;
    sx += x, sy += y;
    lox = fminf(lox, x), loy = fminf(loy, y);
  }
  const float shx = lox > -1e-12f ? 0.0f : 1.0f, shy = loy > -1e-12f ? 0.0f : 1.0f;   // graph_datastruct.py:696-704
  const float cx = sx / (float)n + shx, cy = sy / (float)n + shy;
  float acc = 0.0f;
  for (int i = lane; i < n; i += 64) {
    int ji = 0;
    float xi = 0.0f, yi = 0.0f;
    if (PERIODIC) {
      for (int k = 0; k <= i; ++k) {
        I.load(p0 + k, j, x, y);
        if (k > 0) x = min_image(x, xi), y = min_image(y, yi);
        xi = x, yi = y, ji = j;
      }
    } else {
      I.load(p0 + i, ji, xi, yi);
    }
    xi += shx, yi += shy;
    PolyScan S;
    S.start(xi - cx, yi - cy, i);
    for (int k = 0; k < n; ++k) {
      I.load(p0 + k, j, x, y);
      if (PERIODIC && k > 0) x = min_image(x, px), y = min_image(y, py);
      px = x, py = y;
      S.see((x + shx) - cx, (y + shy) - cy, k);
    }
    const int64_t at = reversed ? p0 + (n - 1 - S.rank) : p0 + S.rank;
    O.joint[at] = ji;
    O.xy[2 * at] = xi;
    O.xy[2 * at + 1] = yi;
    float fx, fy;
    S.follower(fx, fy);
    acc += (xi - cx) * fy - (yi - cy) * fx;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
  if (lane == 0) {
    O.centre[2 * g] = cx;
    O.centre[2 * g + 1] = cy;
    O.area[g] = (reversed ? -0.5f : 0.5f) * acc;
  }
}

// Is `g` the first grain of a trajectory that has grains (the no-flux boundary grain of its trajectory)?
__device__ __forceinline__ bool poly_boundary_grain(const int64_t* __restrict__ off, int64_t n_traj, int64_t g) {
  if (off == nullptr) return g == 0;
  int64_t a = 0, z = n_traj;   // the last t in [0, n_traj] with off[t] <= g (off[0] = 0)
  while (a < z) {
    const int64_t m = (a + z + 1) >> 1;
    if (off[m] <= g) a = m; else z = m - 1;
  }
  return a < n_traj && off[a] == g;
}

template <bool PERIODIC>
__global__ __launch_bounds__(POLY_BLOCK) void grain_polygons_kernel(const ggnn_polygon_args A) {
  const int tid = threadIdx.x, lane = tid & 63, l = tid & (POLY_GROUP - 1);
  // the layer this launch writes: read by every block before the last one to finish advances the counter
  const int64_t k = A.layer_in ? (int64_t)*A.layer_in + 1 : 0;
  const bool room = k >= 0 && k <= A.capacity;
  const int64_t g = (int64_t)blockIdx.x * POLY_GRAINS + (tid >> 4);
  if (room) {   // (block-uniform)
    const PolyIn I = {A.col, A.x_joint, A.domain_offset, A.ldx_joint, A.n_joint, A.domain_factor};
    const PolyOut O = {A.joint_sorted + k * A.E_cap, A.xy_sorted + 2 * k * A.E_cap, A.centre + 2 * k * A.n_grain,
                       A.area + k * A.n_grain};
    int32_t* rowptr_out = A.rowptr_out + k * (A.n_grain + 1);
    int p0 = 0, n = 0;
    bool reversed = false;
    if (g < A.n_grain) {
      const int32_t r0 = A.rowptr[g], r1 = A.rowptr[g + 1];
      p0 = (int)min((int64_t)max(r0, 0), A.E_cap);   // nothing outside [0, E_cap) is addressed, whatever the table holds
      n = (int)min((int64_t)max(r1, p0), A.E_cap) - p0;
      if (l == 0) {
        rowptr_out[g] = r0;
        if (g == A.n_grain - 1) rowptr_out[g + 1] = r1;
      }
      if (!PERIODIC) reversed = poly_boundary_grain(A.traj_grain_off, A.n_traj, g);   // graph_datastruct.py:715-716
      if (n <= 1 && l == 0) poly_short_row(I, O, g, p0, n);
    }
    // -- rows of 2..16 junctions: lane l of the group holds vertex l ------------------------------------------------------
    const int m = n >= 2 && n <= POLY_GROUP ? n : 0;
    const bool have = l < m;
    int j = 0;
    float x = 0.0f, y = 0.0f;
    if (have) I.load(p0 + l, j, x, y);
    float px = 0.0f, py = 0.0f, sx = 0.0f, sy = 0.0f, lox = INFINITY, loy = INFINITY;
    for (int v = 0; __any(v < m); ++v) {   // (the same trip count in every lane of the wave: the shuffles see all lanes)
      if (PERIODIC && v > 0 && l == v && have) x = min_image(x, px), y = min_image(y, py);
      px = __shfl(x, v, POLY_GROUP);
      py = __shfl(y, v, POLY_GROUP);
      if (v < m) {
        sx += px, sy += py;
        lox = fminf(lox, px), loy = fminf(loy, py);
      }
    }
    const float shx = lox > -1e-12f ? 0.0f : 1.0f, shy = loy > -1e-12f ? 0.0f : 1.0f;
    const float cx = m ? sx / (float)m + shx : 0.0f, cy = m ? sy / (float)m + shy : 0.0f;
    x += shx, y += shy;
    const float dx = x - cx, dy = y - cy;
    PolyScan S;
    S.start(dx, dy, l);
    for (int v = 0; __any(v < m); ++v) {
      const float vx = __shfl(dx, v, POLY_GROUP), vy = __shfl(dy, v, POLY_GROUP);
      if (v < m) S.see(vx, vy, v);
    }
    float cross = 0.0f;
    if (have) {
      const int64_t at = reversed ? p0 + (m - 1 - S.rank) : p0 + S.rank;
      O.joint[at] = j;
      O.xy[2 * at] = x;
      O.xy[2 * at + 1] = y;
      float fx, fy;
      S.follower(fx, fy);
      cross = dx * fy - dy * fx;
    }
    cross = row_sum(cross);
    if (m && l == 0) {
      O.centre[2 * g] = cx;
      O.centre[2 * g + 1] = cy;
      O.area[g] = (reversed ? -0.5f : 0.5f) * cross;
    }
    // -- longer rows: one at a time, by the whole wave ---------------------------------------------------------------------
    if (__any(n > POLY_GROUP)) {
#pragma unroll 1
      for (int q = 0; q < 64 / POLY_GROUP; ++q) {
        const int nq = __builtin_amdgcn_readfirstlane(__shfl(n, q * POLY_GROUP));
        const int pq = __builtin_amdgcn_readfirstlane(__shfl(p0, q * POLY_GROUP));
        const int rq = __builtin_amdgcn_readfirstlane(__shfl((int)reversed, q * POLY_GROUP));
        if (nq > POLY_GROUP) poly_row_wave<PERIODIC>(I, O, g - (tid >> 4 & 3) + q, pq, nq, rq != 0, lane);
      }
    }
  }
  // the last block to get here has seen every other block read the counter
  if (A.layer_out != nullptr) {
    __syncthreads();
    if (tid == 0) {
      __threadfence();
      if (atomicAdd(A.sync_word, 1) == (int32_t)gridDim.x - 1) {
        *A.sync_word = 0;
        *A.layer_out = (int32_t)min(k, (int64_t)INT32_MAX);
        if (!room) atomicOr(A.flags, GGNN_FLAG_POLYGON_OVERFLOW);
      }
    }
  }
}

}  // namespace ggnn

extern "C" int ggnn_grain_polygons(const ggnn_polygon_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_polygon_args& A = *args;
  if (A.boundary != GGNN_BC_PERIODIC && A.boundary != GGNN_BC_NOFLUX) return GGNN_EINVAL;
  if (!A.rowptr || !A.col || !A.x_joint || !A.rowptr_out || !A.joint_sorted || !A.xy_sorted || !A.centre || !A.area)
    return GGNN_EINVAL;
  if (A.n_joint <= 0 || A.n_grain <= 0 || A.ldx_joint < 2 || A.E_cap < 0 || A.E_cap >= INT32_MAX) return GGNN_EINVAL;
  if (!(A.domain_factor >= 1.0f) || A.capacity < 0 || A.capacity >= INT32_MAX) return GGNN_EINVAL;
  if (A.traj_grain_off ? A.n_traj < 1 || A.n_traj > (1 << 29) : A.n_traj != 1) return GGNN_EINVAL;
  if (A.layer_out && (!A.sync_word || !A.flags)) return GGNN_EINVAL;
  const int64_t nblk = (A.n_grain + POLY_GRAINS - 1) / POLY_GRAINS;
  if (nblk >= INT32_MAX) return GGNN_EINVAL;
  const auto kernel = A.boundary == GGNN_BC_PERIODIC ? grain_polygons_kernel<true> : grain_polygons_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(POLY_BLOCK), 0, (hipStream_t)stream, A);
  return launch_status();
}
