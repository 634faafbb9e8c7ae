// The grain-ID image of recorded layers: the polygons ggnn_grain_polygons left in its arena (polygons.hip), filled as the
// reference's plot_polygons does (graph_datastruct.py:553-610) -- `alpha_field`, the map its misclassification rate, its
// initial areas and its 3-D reconstruction are made from.
//   ggnn_polygons_rasterize = a batch of layers, one launch: image[l][y][x] = the highest grain index + 1 among the polygons
//                             of layer l whose closed integer polygon holds the lattice point (x, y); 0 = uncovered
//   ggnn_image_compare      = the differing pixels of an image and a second one, and the pixel count of every id
// The rule is exact in integers (include/ggnn.h; tests/rastercheck.py restates it by brute force):
//   vertices   v = (int)(x * (float)s), periodic, or (int)rintf(x * (float)s), no-flux: ONE fp32 product (nothing to
//              contract it with), saturated at +-2^20 so that every difference of two coordinates fits 22 bits
//   membership on an edge, or an odd number of crossings under the half-open rule in y
//   ownership  atomicMax of grain index + 1: independent of the order, so of the grid
// One wave takes one polygon.  A lane holds edge e = (vertex e, vertex e + 1) of the row on one scanline y, oriented a -> b
// with ya < yb, and its crossing with the scanline as an exact rational
//     xc = xa + num / den,   num = (y - ya) (xb - xa)  (int64: up to 2^43),   den = yb - ya > 0
// rounded both ways.  With q = num / den truncated toward zero and r = num - q den (C++'s / and %: r has num's sign),
//     floor(num / den) = q - (r < 0),   ceil(num / den) = q + (r > 0)
// -- for a negative numerator truncation rounds UP, so the floor takes the correction and the ceiling none.  From
// cf = xa + floor and cc = xa + ceil a pixel x decides without another product:
//     strictly left of the edge   x < xc  <=>  x < cc            (counted for ya <= y < yb: the half-open rule)
//     on the edge                 x = xc  <=>  cc <= x <= cf     (possible only where the division is exact; ya <= y <= yb)
//     on a horizontal edge at y           <=>  min(xa, xb) <= x <= max(xa, xb)
// which is the sign of the cross product (x - xa) den - num in each case.
// A vector instruction costs the same whether 6 lanes or 64 do something, so a row of n <= 64 junctions fills the wave with
// 64 / n scanlines at once: lane r n + e works out edge e on scanline yb + r, ten scanlines of a hexagon in one pass.  Two
// ballots say which lanes hold an edge that counts and which hold one with pixels ON it; then, scanline by scanline, the
// lanes run along x -- a wave's atomics are one contiguous run of the image's row -- and every pixel looks only at the
// edges its scanline's bits name, fetched through v_readlane with a uniform index (no LDS, no shuffle): two compares a
// scanline for a convex polygon, whatever its row's length.  The run is the polygon's box where that is at most 64 pixels
// wide (one run either way); a wider polygon's scanline takes its span [min cf, max cc] over the edges that touch it,
// clipped to the canvas.  Rows of more than 64 junctions take one scanline at a time and the edges in chunks of 64, computed
// again for every run of 64 pixels: nothing needs scratch, any length is correct.
// Every index is clamped as in polygons.hip: whatever the tables hold, nothing outside the arena rows and the image is
// addressed, and the work per polygon is bounded by the canvas.
#include <algorithm>

#include "common.h"
#include "segments.h"

namespace ggnn {

constexpr int RASTER_BLOCK = 256;                    // four waves, one polygon each
constexpr int RASTER_WAVES = RASTER_BLOCK / 64;
constexpr float RASTER_SATURATE = 1048576.0f;        // 2^20

struct RasterLayers {
  int32_t at[GGNN_RASTER_MAX_LAYERS];
};

template <bool PERIODIC>
__device__ __forceinline__ int raster_vertex(float x, float s) {
  float p = __fmul_rn(x, s);
  if (!PERIODIC) p = rintf(p);
  p = fminf(fmaxf(p, -RASTER_SATURATE), RASTER_SATURATE);   // (NaN -> -2^20, as numpy's fmax / fmin)
  return (int)p;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
  return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m));
  return __builtin_amdgcn_readfirstlane(v);
}

// One edge on one scanline: `left` = pixels x < left are strictly left of it (INT_MIN: not counted), [lo, hi] = the pixels
// on it (empty: lo > hi), [from, to] = what it adds to the scanline's span (none: from > to).
struct RasterEdge {
  int left, lo, hi, from, to;
};

__device__ __forceinline__ RasterEdge raster_edge(bool have, int x0, int y0, int x1, int y1, int y) {
  RasterEdge E = {INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN};
  if (!have) return E;
  if (y0 == y1) {
    if (y == y0) E.lo = E.from = min(x0, x1), E.hi = E.to = max(x0, x1);
    return E;
  }
  const bool up = y0 < y1;
  const int xa = up ? x0 : x1, ya = up ? y0 : y1, xb = up ? x1 : x0, yb = up ? y1 : y0;
  if (y < ya || y > yb) return E;
  const int64_t num = (int64_t)(y - ya) * (int64_t)(xb - xa);
  const int den = yb - ya;
  int q, r;   // truncated quotient and the remainder's sign
  if (num == (int64_t)(int32_t)num) {
    q = (int32_t)num / den;
    const int rem = (int32_t)num - q * den;
    r = (rem > 0) - (rem < 0);
  } else {
    const int64_t q64 = num / den, rem = num - q64 * den;
    q = (int)q64;   // |num / den| <= |xb - xa| < 2^22
    r = (rem > 0) - (rem < 0);
  }
  const int cf = xa + q - (r < 0 ? 1 : 0), cc = xa + q + (r > 0 ? 1 : 0);
  E.left = y < yb ? cc : INT32_MIN;
  E.lo = cc, E.hi = cf;
  E.from = cf, E.to = cc;
  return E;
}

template <bool PERIODIC>
__global__ __launch_bounds__(RASTER_BLOCK) void polygons_rasterize_kernel(const ggnn_raster_args A, const RasterLayers layers,
                                                                          int first) {
  const int lane = threadIdx.x & 63;
  // one polygon per wave: everything below that does not name `lane` or `x` is wave-uniform, and said to be so
  const int64_t g = A.grain_begin + (int64_t)blockIdx.x * RASTER_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (g >= A.grain_end) return;
  if (!PERIODIC && seg_is_first(A.traj_grain_off, (int)A.n_traj, g)) return;   // (a trajectory's boundary grain is not drawn)
  const int64_t k = min((int64_t)max(layers.at[blockIdx.y], 0), A.capacity);
  const int32_t* __restrict__ rowptr = A.rowptr + k * (A.n_grain + 1);
  const float* __restrict__ xy = A.xy_sorted + 2 * k * A.E_cap;
  const int p0 = __builtin_amdgcn_readfirstlane((int)min((int64_t)max(rowptr[g], 0), A.E_cap));
  const int n = __builtin_amdgcn_readfirstlane((int)min((int64_t)max(rowptr[g + 1], p0), A.E_cap)) - p0;
  if (n < 2) return;
  const int nx = (int)A.nx, ny = (int)A.ny;
  const int width = PERIODIC ? 2 * nx : nx, height = PERIODIC ? 2 * nx : ny;   // the canvas
  const float s = (float)nx;
  int32_t* __restrict__ image = A.image + ((int64_t)first + blockIdx.y) * (PERIODIC ? (int64_t)nx * nx : (int64_t)ny * nx);
  const int32_t id = (int32_t)(g - A.grain_begin) + 1;

  // edge e of the row: vertices e and e + 1 (the last one closes the polygon)
  auto load_edge = [&](int e, int& x0, int& y0, int& x1, int& y1) {
    const int64_t a = p0 + min(e, n - 1), b = p0 + (e + 1 < n ? e + 1 : 0);
    x0 = raster_vertex<PERIODIC>(xy[2 * a], s), y0 = raster_vertex<PERIODIC>(xy[2 * a + 1], s);
    x1 = raster_vertex<PERIODIC>(xy[2 * b], s), y1 = raster_vertex<PERIODIC>(xy[2 * b + 1], s);
  };
  auto put = [&](int x, int fy) {
    const int fx = PERIODIC && x >= nx ? x - nx : x;
    atomicMax(image + (int64_t)fy * nx + fx, id);   // (the old value is not used: an atomic without return)
  };
  const int chunks = (n + 63) >> 6;
  // -- rows of up to 64 junctions: `rows` = 64 / n scanlines at a time, lane r n + e holding edge e on scanline yb + r -------
  const int rows = chunks == 1 ? 64 / n : 0;
  const int r = chunks == 1 ? lane / n : 0, e = lane - r * n;
  int x0, y0, x1, y1;
  int ylo = INT32_MAX, yhi = INT32_MIN, bxlo = INT32_MAX, bxhi = INT32_MIN;   // the polygon's box
  for (int c = chunks - 1; c >= 0; --c) {
    load_edge(c * 64 + lane, x0, y0, x1, y1);
    if (c * 64 + lane < n) ylo = min(ylo, y0), yhi = max(yhi, y0), bxlo = min(bxlo, x0), bxhi = max(bxhi, x0);
  }
  ylo = max(wave_min(ylo), 0), yhi = min(wave_max(yhi), height - 1);
  bxlo = max(wave_min(bxlo), 0), bxhi = min(wave_max(bxhi), width - 1);
  // A box of up to 64 pixels is one run of the lanes whatever the scanline's span is: the span is worked out only for
  // polygons wider than that.
  const bool narrow = bxhi - bxlo < 64;
  if (chunks == 1) {
    load_edge(e, x0, y0, x1, y1);
    const uint64_t row_mask = n == 64 ? ~0ull : (1ull << n) - 1;
#pragma unroll 1
    for (int yb = ylo; yb <= yhi; yb += rows) {
      // the edges of `rows` scanlines in one pass; which of them count and which hold pixels at all is a mask each, so the
      // pixels below look only at those -- a convex polygon's scanline has two counting edges, whatever its row's length
      const RasterEdge E = raster_edge(r < rows && yb + r <= yhi, x0, y0, x1, y1, yb + r);
      const uint64_t counting = __ballot(E.left != INT32_MIN), holding = __ballot(E.lo <= E.hi);
      const int last = min(rows, yhi - yb + 1);
#pragma unroll 1
      for (int q = 0; q < last; ++q) {
        const int l0 = q * n, y = yb + q;
        const uint64_t cm = (counting >> l0) & row_mask, hm = (holding >> l0) & row_mask;
        int xlo = bxlo, xhi = bxhi;
        if (!narrow) {   // the scanline's span: [min floor, max ceil] of its edges' crossings
          int from = INT32_MAX, to = INT32_MIN;
          for (int i = 0; i < n; ++i)
            from = min(from, __builtin_amdgcn_readlane(E.from, l0 + i)), to = max(to, __builtin_amdgcn_readlane(E.to, l0 + i));
          xlo = max(from, 0), xhi = min(to, width - 1);
        }
        const int fy = PERIODIC && y >= nx ? y - nx : y;
#pragma unroll 1
        for (int base = xlo; base <= xhi; base += 64) {
          const int x = base + lane;
          bool odd = false, on = false;
          for (uint64_t m = cm; m; m &= m - 1) odd ^= x < __builtin_amdgcn_readlane(E.left, l0 + __builtin_ctzll(m));
          for (uint64_t m = hm; m; m &= m - 1) {
            const int l = l0 + __builtin_ctzll(m);
            on |= x >= __builtin_amdgcn_readlane(E.lo, l) && x <= __builtin_amdgcn_readlane(E.hi, l);
          }
          if ((odd || on) && x <= xhi) put(x, fy);
        }
      }
    }
    return;
  }
  // -- longer rows: one scanline at a time, the edges in chunks of 64, computed again for every run of 64 pixels --------------
#pragma unroll 1
  for (int y = ylo; y <= yhi; ++y) {
    RasterEdge E;
    int from = INT32_MAX, to = INT32_MIN;
    for (int c = 0; c < chunks; ++c) {
      load_edge(c * 64 + lane, x0, y0, x1, y1);
      E = raster_edge(c * 64 + lane < n, x0, y0, x1, y1, y);
      from = min(from, E.from), to = max(to, E.to);
    }
    const int xlo = max(wave_min(from), 0), xhi = min(wave_max(to), width - 1);
    const int fy = PERIODIC && y >= nx ? y - nx : y;
#pragma unroll 1
    for (int base = xlo; base <= xhi; base += 64) {
      const int x = base + lane;
      bool odd = false, on = false;
      for (int c = 0; c < chunks; ++c) {
        load_edge(c * 64 + lane, x0, y0, x1, y1);
        E = raster_edge(c * 64 + lane < n, x0, y0, x1, y1, y);
        const int m = min(n - c * 64, 64);
#pragma unroll 1
        for (int i = 0; i < m; ++i) {
          const int left = __builtin_amdgcn_readlane(E.left, i);
          const int lo = __builtin_amdgcn_readlane(E.lo, i), hi = __builtin_amdgcn_readlane(E.hi, i);
          odd ^= x < left;
          on |= x >= lo && x <= hi;
        }
      }
      if ((odd || on) && x <= xhi) put(x, fy);
    }
  }
}

// Uncovered pixels of a no-flux image take their quadrant's corner grain (graph_datastruct.py:602-605).
__global__ __launch_bounds__(256) void raster_corner_fill_kernel(int32_t* __restrict__ image, int64_t n_layers, int nx, int ny,
                                                                 int c0, int c1, int c2, int c3) {
  const int64_t per = (int64_t)nx * ny, total = per * n_layers;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (image[i] != 0) continue;
    const int64_t p = i % per;
    const int x = (int)(p % nx), y = (int)(p / nx);
    const int patch = 2 * x / nx + 2 * (2 * y / ny);
    image[i] = patch == 0 ? c0 : patch == 1 ? c1 : patch == 2 ? c2 : c3;
  }
}

// Every block takes one contiguous piece of the image, four neighbouring pixels a thread and step, equal ones counted
// together.  LOCAL: the counts go to a histogram of the block's own in LDS (32-bit: a piece has fewer than 2^31 pixels) and
// only the ids the piece holds -- a few hundred of the benchmark's 10 000 -- reach the 64-bit counts, once a block: one
// global atomic per run took 1 082 us on the benchmark's 21 M pixels, this form 88 us.  Not LOCAL (more ids than
// the LDS holds): one global atomic per run.  The differing pixels are summed per wave, then one atomic.
constexpr int COMPARE_BLOCK = 256;
constexpr int64_t COMPARE_LOCAL_IDS = 12 * 1024;   // 48 KB of LDS

template <bool LOCAL>
__global__ __launch_bounds__(COMPARE_BLOCK) void image_compare_kernel(const int32_t* __restrict__ image,
                                                                     const int32_t* __restrict__ truth, int64_t n, int64_t piece,
                                                                     int64_t n_id, unsigned long long* __restrict__ differing,
                                                                     unsigned long long* __restrict__ counts) {
  extern __shared__ uint32_t local[];
  const bool count = counts != nullptr;
  if (LOCAL && count) {
    for (int64_t b = threadIdx.x; b < n_id; b += COMPARE_BLOCK) local[b] = 0;
    __syncthreads();
  }
  auto add = [&](int32_t id, int32_t len) {
    if (!count || id < 0 || id >= n_id) return;
    if (LOCAL) atomicAdd(local + id, (uint32_t)len);
    else atomicAdd(counts + id, (unsigned long long)len);
  };
  const int64_t begin = (int64_t)blockIdx.x * piece, end = min(begin + piece, n);
  unsigned long long diff = 0;
  for (int64_t i = begin + 4 * (int64_t)threadIdx.x; i < end; i += 4 * COMPARE_BLOCK) {
    const int m = (int)min((int64_t)4, end - i);
    int32_t run = 0, len = 0;
    for (int j = 0; j < m; ++j) {
      const int32_t v = image[i + j];
      if (truth != nullptr) diff += v != truth[i + j] ? 1 : 0;
      if (len && v != run) add(run, len), len = 0;
      run = v, ++len;
    }
    if (len) add(run, len);
  }
  if (LOCAL && count) {
    __syncthreads();
    for (int64_t b = threadIdx.x; b < n_id; b += COMPARE_BLOCK) {
      const uint32_t c = local[b];
      if (c) atomicAdd(counts + b, (unsigned long long)c);
    }
  }
  if (truth != nullptr) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) diff += __shfl_xor(diff, m);
    if ((threadIdx.x & 63) == 0 && diff) atomicAdd(differing, diff);
  }
}

}  // namespace ggnn

extern "C" int ggnn_polygons_rasterize(const ggnn_raster_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_raster_args& A = *args;
  if (A.boundary != GGNN_BC_PERIODIC && A.boundary != GGNN_BC_NOFLUX) return GGNN_EINVAL;
  if (!A.rowptr || !A.xy_sorted || !A.image) return GGNN_EINVAL;
  if (A.nx <= 0 || A.ny <= 0 || A.nx >= (1 << 15) || A.ny >= (1 << 15)) return GGNN_EINVAL;
  if (A.n_grain <= 0 || A.E_cap < 0 || A.E_cap >= INT32_MAX || A.capacity < 0 || A.capacity >= INT32_MAX) return GGNN_EINVAL;
  if (A.grain_begin < 0 || A.grain_end < A.grain_begin || A.grain_end > A.n_grain) return GGNN_EINVAL;
  if (!seg_union_ok(A.traj_grain_off, A.n_traj, true)) return GGNN_EINVAL;
  if (A.n_layers <= 0 || A.n_layers >= INT32_MAX) return GGNN_EINVAL;
  for (int64_t l = 0; l < A.n_layers; ++l) {
    const int64_t k = A.layers ? (int64_t)A.layers[l] : l;
    if (k < 0 || k > A.capacity) return GGNN_EINVAL;
  }
  const bool periodic = A.boundary == GGNN_BC_PERIODIC;
  const int64_t per = periodic ? A.nx * A.nx : A.nx * A.ny;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(A.image, 0, (size_t)(per * A.n_layers) * sizeof(int32_t), st) != hipSuccess) return GGNN_ELAUNCH;
  const int64_t nblk = (A.grain_end - A.grain_begin + RASTER_WAVES - 1) / RASTER_WAVES;
  if (nblk >= INT32_MAX) return GGNN_EINVAL;
  const auto kernel = periodic ? polygons_rasterize_kernel<true> : polygons_rasterize_kernel<false>;
  for (int64_t first = 0; nblk > 0 && first < A.n_layers; first += GGNN_RASTER_MAX_LAYERS) {   // one launch up to the table's size
    RasterLayers L;
    const int m = (int)std::min<int64_t>(GGNN_RASTER_MAX_LAYERS, A.n_layers - first);
    for (int l = 0; l < GGNN_RASTER_MAX_LAYERS; ++l) L.at[l] = l < m ? (A.layers ? A.layers[first + l] : (int32_t)(first + l)) : 0;
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblk, (unsigned)m), dim3(RASTER_BLOCK), 0, st, A, L, (int)first);
  }
  if (!periodic && A.with_corners) {
    const int64_t blocks = std::min<int64_t>((per * A.n_layers + 255) / 256, 64 * 1024);
    hipLaunchKernelGGL(raster_corner_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, st, A.image, A.n_layers, (int)A.nx,
                       (int)A.ny, A.corner_grains[0], A.corner_grains[1], A.corner_grains[2], A.corner_grains[3]);
  }
  return launch_status();
}

extern "C" int ggnn_image_compare(const int32_t* image, const int32_t* truth, int64_t n_pixels, int64_t n_grain,
                                  uint64_t* differing, uint64_t* counts, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!image || n_pixels <= 0 || n_grain < 0 || n_grain >= INT32_MAX) return GGNN_EINVAL;
  if ((truth != nullptr) != (differing != nullptr) || (!truth && !counts)) return GGNN_EINVAL;
  // pieces of whole steps of a block, at most 2^30 pixels each, four blocks a compute unit (what its LDS holds of them) where the image has that many
  const int64_t step = 4 * COMPARE_BLOCK, steps = (n_pixels + step - 1) / step;
  const int64_t want = std::max<int64_t>(4 * (int64_t)num_cu(), (n_pixels >> 30) + 1);
  const int64_t piece = (steps + std::min(want, steps) - 1) / std::min(want, steps) * step;
  const int64_t blocks = (n_pixels + piece - 1) / piece;
  if (blocks >= INT32_MAX) return GGNN_EINVAL;
  const int64_t n_id = n_grain + 1;
  if (counts && n_id <= COMPARE_LOCAL_IDS)
    hipLaunchKernelGGL(image_compare_kernel<true>, dim3((unsigned)blocks), dim3(COMPARE_BLOCK), (size_t)n_id * sizeof(uint32_t),
                       (hipStream_t)stream, image, truth, n_pixels, piece, n_id, (unsigned long long*)differing,
                       (unsigned long long*)counts);
  else
    hipLaunchKernelGGL(image_compare_kernel<false>, dim3((unsigned)blocks), dim3(COMPARE_BLOCK), 0, (hipStream_t)stream, image,
                       truth, n_pixels, piece, n_id, (unsigned long long*)differing, (unsigned long long*)counts);
  return launch_status();
}
