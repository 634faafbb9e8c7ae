// The row code of the grains' junction polygons, shared by the two kernels that build polygon records so that they cannot
// drift: ggnn_grain_polygons (polygons.hip: a layer of the rollout's own state) and ggnn_interp_polygons (interp.hip: a
// layer blended from two recorded ones).  The rule is include/ggnn.h's, ggnn_grain_polygons; polygons.hip describes the key
// and the two row paths.
#pragma once
#include "common.h"
#include "segments.h"

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
  // junction jj's xy in the global frame (test.py:474)
  __device__ __forceinline__ void global_xy(int64_t jj, float& x, float& y) const {
    x = x_joint[jj * ldxj];
    y = x_joint[jj * ldxj + 1];
    if (factor > 1.0f) {
      x = (x + (offset ? offset[2 * jj] : 0.0f)) / factor;
      y = (y + (offset ? offset[2 * jj + 1] : 0.0f)) / factor;
    }
  }
  // vertex `at` of the table: its junction and the junction's xy in the global frame
  __device__ __forceinline__ void load(int at, int& j, float& x, float& y) const {
    const int64_t jj = min((int64_t)max(col[at], 0), n_joint - 1);
    j = (int)jj;
    global_xy(jj, x, y);
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

// The grains of one block, POLY_GRAINS of them from blockIdx.x * POLY_GRAINS: their rows of (rowptr, I.col) into O, and a
// copy of rowptr into rowptr_out.  Every thread of the block must call it.
template <bool PERIODIC>
__device__ __forceinline__ void poly_block_rows(const PolyIn& I, const PolyOut& O, const int32_t* __restrict__ rowptr,
                                                int32_t* __restrict__ rowptr_out, int64_t n_grain, int64_t E_cap,
                                                const int64_t* __restrict__ traj_grain_off, int64_t n_traj) {
  const int tid = threadIdx.x, lane = tid & 63, l = tid & (POLY_GROUP - 1);
  const int64_t g = (int64_t)blockIdx.x * POLY_GRAINS + (tid >> 4);
  int p0 = 0, n = 0;
  bool reversed = false;
  if (g < n_grain) {
    const int32_t r0 = rowptr[g], r1 = rowptr[g + 1];
    p0 = (int)min((int64_t)max(r0, 0), E_cap);   // nothing outside [0, E_cap) is addressed, whatever the table holds
    n = (int)min((int64_t)max(r1, p0), E_cap) - p0;
    if (l == 0) {
      rowptr_out[g] = r0;
      if (g == n_grain - 1) rowptr_out[g + 1] = r1;
    }
    if (!PERIODIC) reversed = seg_is_first(traj_grain_off, (int)n_traj, g);   // a boundary grain, graph_datastruct.py:715-716
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

}  // namespace ggnn
