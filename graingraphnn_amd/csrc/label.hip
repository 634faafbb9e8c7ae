// Segment an orientation map (or a noisy id image) into a grain-ID image: connected components of the pixel-to-pixel links,
// specks and non-indexed pixels dissolved into their neighbours, canonical numbering, per-grain mean angles.  The rule is
// include/ggnn.h's (ggnn_label_grains), restated by tests/labelcheck.py; everything here is exact in integers.
//
//   links     a byte a pixel: linked right, linked down, valid                               (either input form, read once)
//   tiles     a workgroup a GGNN_LABEL_TILE_X x GGNN_LABEL_TILE_Y tile: union-find on LDS labels, the tile-local roots
//             written as global raster indices, their pixel counts and fixed-point angle sums accumulated in LDS
//   seams     a thread a linked pair across a tile edge or the periodic wrap: atomicMin on the larger root's parent, retried
//   flatten   every pixel's root; a tile-local root folds its count and sums into the root (one atomic a tile-local component)
//   classify  closed / open, every chunk of 1 024 pixels lists its open pixels in its own stretch of the list, the counters
//   sweeps    decide (from the state before the sweep, into a side array) and commit, 2 max_sweeps launches; a sweep after
//             one that assigned nothing returns on a device word
//   rank      block sums, scan of the sums, add (and the means, at the roots); then the image
//
// ggnn_label_orientations (full orientations under cubic symmetry; tests/orientcheck.py) runs the same stages with K = 0 behind
// a links kernel of its own (the disorientation of two quaternions in closed form), and adds three launches: the sums zeroed at
// the roots and every closed pixel aligned to its root and accumulated (after classify), the means normalised (after the rank).
//
// No kernel waits on another workgroup: the order between workgroups is the order of the launches.  Every loop that follows
// parents carries a budget of hops derived from the number of pixels; a thread that spends it counts itself in n_bound_hits
// and leaves.  Parent words that another workgroup may write in the same launch (the seam merge) are read and written with
// agent-scope atomics alone.
#include <algorithm>

#include "common.h"

namespace ggnn {

constexpr int LABEL_TX = GGNN_LABEL_TILE_X, LABEL_TY = GGNN_LABEL_TILE_Y;
constexpr int LABEL_TILE = LABEL_TX * LABEL_TY;          // 1024 pixels: 256 threads, four neighbouring pixels each
constexpr int LABEL_BLOCK = 256;
constexpr int LABEL_PER_THREAD = LABEL_TILE / LABEL_BLOCK;
constexpr int SCAN_CHUNK = 4 * LABEL_BLOCK;
constexpr uint8_t LINK_RIGHT = 1, LINK_DOWN = 2, LINK_VALID = 4, LINK_LOCAL_ROOT = 8;
enum { ST_COMPONENTS, ST_SPECKS, ST_SPECK_PIXELS, ST_INVALID_IN, ST_GRAINS, ST_SWEEPS, ST_UNFILLED, ST_OVERFLOW, ST_BOUND_HITS };
static_assert(LABEL_TX % LABEL_PER_THREAD == 0 && LABEL_TILE % LABEL_BLOCK == 0, "a thread's pixels lie in one row of the tile");
static_assert(ST_BOUND_HITS + 1 == GGNN_LABEL_STATUS_WORDS, "the status words of include/ggnn.h");

struct LabelWs {          // the carved workspace
  int32_t* words;         // [1 + s] the pixels sweep s assigned ([0] spare)
  uint8_t* links;         // [N]
  int32_t* parent;        // [N]; dead after flatten: the sweeps' side array lives here
  uint32_t* size;         // [N], at roots
  int32_t* lab;           // [N]: the root of a closed pixel, -1 open
  int32_t* list;          // [N]: the open pixels of chunk c of SCAN_CHUNK pixels at c SCAN_CHUNK .. + open[c]
  int32_t* open;          // [chunks]
  int32_t* rank;          // [N], at grain roots
  int32_t* bsum;          // [chunks]
  long long* sums;        // [K, N], at roots
};
constexpr size_t LABEL_ALIGN = 256;
static inline size_t up(size_t b) { return (b + LABEL_ALIGN - 1) / LABEL_ALIGN * LABEL_ALIGN; }
static inline size_t label_words_bytes() { return up((size_t)(GGNN_LABEL_MAX_SWEEPS + 1) * sizeof(int32_t)); }
static size_t label_carve(LabelWs* w, char* base, int64_t N, int K) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += up(bytes);
    return p;
  };
  const size_t n = (size_t)N, chunks = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
  char* words = take(label_words_bytes());
  char* links = take(n);
  char* parent = take(4 * n);
  char* size = take(4 * n);
  char* lab = take(4 * n);
  char* list = take(4 * n);
  char* rank = take(4 * n);
  char* bsum = take(4 * chunks);
  char* open = take(4 * chunks);
  char* sums = take(8 * n * (size_t)K);
  if (w) *w = LabelWs{(int32_t*)words, (uint8_t*)links, (int32_t*)parent, (uint32_t*)size, (int32_t*)lab, (int32_t*)list,
                      (int32_t*)open, (int32_t*)rank, (int32_t*)bsum, (long long*)sums};
  return o;
}

struct LabelDims {
  int nx, ny, N, K;
  bool periodic;
};

__device__ __forceinline__ void count_to(int64_t* word, unsigned long long v) {   // a sum over the wave, one atomic
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long*)word, v);
}

// ---- links -------------------------------------------------------------------------------------------------------------------
template <bool ANGLES>
__device__ __forceinline__ bool pixel_valid(const int32_t* ids, const float* angles, const uint8_t* mask, int64_t p, int64_t N, int K) {
  if (mask && !mask[p]) return false;
  if (!ANGLES) return ids[p] >= 1;
  for (int k = 0; k < K; ++k) {
    const float a = angles[(int64_t)k * N + p];
    if (!(fabsf(a) <= 8.0f)) return false;   // (NaN and inf fail the comparison)
  }
  return true;
}
template <bool ANGLES>
__device__ __forceinline__ bool pixels_alike(const int32_t* ids, const float* angles, int64_t p, int64_t q, int64_t N, int K, float tol) {
  if (!ANGLES) return ids[p] == ids[q];
  for (int k = 0; k < K; ++k)
    if (!(fabsf(__fsub_rn(angles[(int64_t)k * N + p], angles[(int64_t)k * N + q])) <= tol)) return false;
  return true;
}

template <bool ANGLES>
__global__ __launch_bounds__(LABEL_BLOCK) void label_links_kernel(const int32_t* __restrict__ ids, const float* __restrict__ angles,
                                                                  const uint8_t* __restrict__ mask, uint8_t* __restrict__ links,
                                                                  LabelDims D, float tol) {
  const int64_t N = D.N;
  for (int64_t p = (int64_t)blockIdx.x * LABEL_BLOCK + threadIdx.x; p < N; p += (int64_t)gridDim.x * LABEL_BLOCK) {
    uint8_t b = 0;
    if (pixel_valid<ANGLES>(ids, angles, mask, p, N, D.K)) {
      b = LINK_VALID;
      const int x = (int)(p % D.nx), y = (int)(p / D.nx);
      if (x + 1 < D.nx || D.periodic) {
        const int64_t q = (int64_t)y * D.nx + (x + 1 < D.nx ? x + 1 : 0);
        if (pixel_valid<ANGLES>(ids, angles, mask, q, N, D.K) && pixels_alike<ANGLES>(ids, angles, p, q, N, D.K, tol)) b |= LINK_RIGHT;
      }
      if (y + 1 < D.ny || D.periodic) {
        const int64_t q = (int64_t)(y + 1 < D.ny ? y + 1 : 0) * D.nx + x;
        if (pixel_valid<ANGLES>(ids, angles, mask, q, N, D.K) && pixels_alike<ANGLES>(ids, angles, p, q, N, D.K, tol)) b |= LINK_DOWN;
      }
    }
    links[p] = b;
  }
}

// ---- tiles: union-find on LDS ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(int* lab, int x, int& budget) {
  while (budget-- > 0) {
    const int p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;
  }
  return -1;
}
// -> false: the budget ran out
__device__ __forceinline__ bool lds_union(int* lab, int a, int b, int& budget) {
  while (budget > 0) {
    a = lds_find(lab, a, budget);
    b = lds_find(lab, b, budget);
    if (a < 0 || b < 0) return false;
    if (a == b) return true;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicMin(lab + a, b);   // a was a root when read: hook it under the smaller root, or follow who was first
    if (old == a) return true;
    a = old;
  }
  return false;
}

__global__ __launch_bounds__(LABEL_BLOCK) void label_tile_kernel(const float* __restrict__ angles, uint8_t* __restrict__ links,
                                                                 int32_t* __restrict__ parent, uint32_t* __restrict__ size,
                                                                 long long* __restrict__ sums, int64_t* __restrict__ status,
                                                                 LabelDims D, int tiles_x) {
  extern __shared__ long long label_lds[];                       // [K][LABEL_TILE] sums, then the labels and the counts
  long long* lsum = label_lds;
  int* lab = (int*)(label_lds + (size_t)D.K * LABEL_TILE);
  unsigned* cnt = (unsigned*)(lab + LABEL_TILE);
  const int x0 = (blockIdx.x % tiles_x) * LABEL_TX, y0 = (blockIdx.x / tiles_x) * LABEL_TY;
  const int first = threadIdx.x * LABEL_PER_THREAD;              // the thread's pixels first .. first + 3 of the tile, one row
  const int ly = first / LABEL_TX, gy = y0 + ly;
  uint8_t b[LABEL_PER_THREAD];
  for (int j = 0; j < LABEL_PER_THREAD; ++j) {
    const int i = first + j, gx = x0 + i % LABEL_TX;
    b[j] = gx < D.nx && gy < D.ny ? links[(int64_t)gy * D.nx + gx] : 0;
    lab[i] = i;
    cnt[i] = 0;
    for (int k = 0; k < D.K; ++k) lsum[k * LABEL_TILE + i] = 0;
  }
  __syncthreads();
  unsigned long long hits = 0;
  for (int j = 0; j < LABEL_PER_THREAD; ++j) {
    const int i = first + j, lx = i % LABEL_TX, gx = x0 + lx;
    // links that stay inside the tile and inside the image (the wrap is a seam)
    if ((b[j] & LINK_RIGHT) && lx + 1 < LABEL_TX && gx + 1 < D.nx) {
      int budget = 4 * LABEL_TILE;
      if (!lds_union(lab, i, i + 1, budget)) ++hits;
    }
    if ((b[j] & LINK_DOWN) && ly + 1 < LABEL_TY && gy + 1 < D.ny) {
      int budget = 4 * LABEL_TILE;
      if (!lds_union(lab, i, i + LABEL_TX, budget)) ++hits;
    }
  }
  __syncthreads();
  int root[LABEL_PER_THREAD];
  for (int j = 0; j < LABEL_PER_THREAD; ++j) {
    int budget = LABEL_TILE;
    root[j] = lds_find(lab, first + j, budget);
    if (root[j] < 0) root[j] = first + j, ++hits;
  }
  for (int j = 0; j < LABEL_PER_THREAD; ++j) {
    if (!(b[j] & LINK_VALID)) continue;
    atomicAdd(cnt + root[j], 1u);
    const int64_t p = (int64_t)gy * D.nx + x0 + (first + j) % LABEL_TX;
    for (int k = 0; k < D.K; ++k) {
      const long long q = __float2ll_rn(__fmul_rn(angles[(int64_t)k * D.N + p], 16777216.0f));
      atomicAdd((unsigned long long*)(lsum + k * LABEL_TILE + root[j]), (unsigned long long)q);
    }
  }
  __syncthreads();
  for (int j = 0; j < LABEL_PER_THREAD; ++j) {
    const int i = first + j, gx = x0 + i % LABEL_TX;
    if (gx >= D.nx || gy >= D.ny) continue;
    const int64_t p = (int64_t)gy * D.nx + gx;
    const int r = root[j];
    parent[p] = (y0 + r / LABEL_TX) * D.nx + x0 + r % LABEL_TX;    // (a root lies inside the image: it is a pixel of it)
    if (r == i) {
      size[p] = cnt[i];
      for (int k = 0; k < D.K; ++k) sums[(int64_t)k * D.N + p] = lsum[k * LABEL_TILE + i];
      if (b[j] & LINK_VALID) links[p] = b[j] | LINK_LOCAL_ROOT;
    }
  }
  count_to(status + ST_BOUND_HITS, hits);
}

// ---- seams: union-find across workgroups -------------------------------------------------------------------------------------
__device__ __forceinline__ int agent_find(int32_t* parent, int x, int64_t& budget) {
  while (budget-- > 0) {
    const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
  return -1;
}

__global__ __launch_bounds__(LABEL_BLOCK) void label_seam_kernel(const uint8_t* __restrict__ links, int32_t* parent,
                                                                 int64_t* __restrict__ status, LabelDims D, int tiles_x, int tiles_y) {
  // the pairs: (right) ny rows x tiles_x last columns, then (down) nx columns x tiles_y last rows
  const int64_t n_right = (int64_t)D.ny * tiles_x, n_all = n_right + (int64_t)D.nx * tiles_y;
  unsigned long long hits = 0;
  for (int64_t t = (int64_t)blockIdx.x * LABEL_BLOCK + threadIdx.x; t < n_all; t += (int64_t)gridDim.x * LABEL_BLOCK) {
    int x, y, x2, y2;
    uint8_t want;
    if (t < n_right) {
      y = (int)(t / tiles_x);
      x = min(((int)(t % tiles_x) + 1) * LABEL_TX, D.nx) - 1;
      x2 = x + 1 < D.nx ? x + 1 : 0, y2 = y, want = LINK_RIGHT;
    } else {
      const int64_t u = t - n_right;
      x = (int)(u / tiles_y);
      y = min(((int)(u % tiles_y) + 1) * LABEL_TY, D.ny) - 1;
      y2 = y + 1 < D.ny ? y + 1 : 0, x2 = x, want = LINK_DOWN;
    }
    if (!(links[(int64_t)y * D.nx + x] & want)) continue;
    int a = y * D.nx + x, b = y2 * D.nx + x2;
    int64_t budget = 2 * (int64_t)D.N + 64;                       // hops of this union, its retries included
    bool done = false;
    while (budget > 0) {
      a = agent_find(parent, a, budget);
      b = agent_find(parent, b, budget);
      if (a < 0 || b < 0) break;
      if (a == b) {
        done = true;
        break;
      }
      if (a < b) {
        const int s = a;
        a = b, b = s;
      }
      const int old = atomicMin(parent + a, b);
      if (old == a) {
        done = true;
        break;
      }
      a = old;                                                     // someone hooked a first: unite what it points to with b
    }
    if (!done) ++hits;
  }
  count_to(status + ST_BOUND_HITS, hits);
}

// ---- flatten, classify -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LABEL_BLOCK) void label_flatten_kernel(const uint8_t* __restrict__ links, const int32_t* __restrict__ parent,
                                                                    uint32_t* size, long long* sums, int32_t* __restrict__ lab,
                                                                    int64_t* __restrict__ status, LabelDims D) {
  unsigned long long hits = 0;
  for (int64_t p = (int64_t)blockIdx.x * LABEL_BLOCK + threadIdx.x; p < D.N; p += (int64_t)gridDim.x * LABEL_BLOCK) {
    int x = (int)p;
    int64_t budget = (int64_t)D.N + 1;
    bool found = false;
    while (budget-- > 0) {                                         // (parents are not written in this launch: plain loads)
      const int up = parent[x];
      if (up == x) {
        found = true;
        break;
      }
      x = up;
    }
    if (!found) x = (int)p, ++hits;
    lab[p] = x;
    if ((links[p] & LINK_LOCAL_ROOT) && x != (int)p) {             // a tile-local component joins its root: one atomic each
      atomicAdd(size + x, size[p]);
      for (int k = 0; k < D.K; ++k)
        atomicAdd((unsigned long long*)(sums + (int64_t)k * D.N + x), (unsigned long long)sums[(int64_t)k * D.N + p]);
    }
  }
  count_to(status + ST_BOUND_HITS, hits);
}

__device__ __forceinline__ int block_exclusive(int mine, int* total, int* wave_sums);

// A workgroup takes chunks of SCAN_CHUNK pixels, four neighbouring ones a thread, and lists a chunk's open pixels in the chunk's
// own stretch of the list, with their number beside it: no counter is shared between workgroups (one atomic a wave of 64 pixels
// on a shared counter cost 0.76 ms of this pass's 1.57 ms at 4 096 x 4 096 with 1 % noise; the 0.81 ms left are not the list's:
// DESIGN 8o).
__global__ __launch_bounds__(LABEL_BLOCK) void label_classify_kernel(const uint8_t* __restrict__ links, const uint32_t* __restrict__ size,
                                                                     int32_t* __restrict__ lab, int32_t* __restrict__ list,
                                                                     int32_t* __restrict__ n_open_of, int64_t* __restrict__ status,
                                                                     LabelDims D, int64_t min_pixels) {
  __shared__ int wave_sums[4];
  unsigned long long comps = 0, specks = 0, speck_px = 0, invalid = 0;
  const int64_t chunks = ((int64_t)D.N + SCAN_CHUNK - 1) / SCAN_CHUNK;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t p0 = c * SCAN_CHUNK + 4 * threadIdx.x;
    bool open[4];
    int n_open = 0;
    for (int j = 0; j < 4; ++j) {
      const int64_t p = p0 + j;
      open[j] = false;
      if (p >= D.N) continue;
      const bool valid = links[p] & LINK_VALID;
      const int r = lab[p];
      const bool closed = valid && (int64_t)size[r] >= min_pixels;
      if (valid && r == (int)p) {
        ++comps;
        if (!closed) ++specks, speck_px += size[r];
      }
      if (!valid) ++invalid;
      lab[p] = closed ? r : -1;
      open[j] = !closed;
      n_open += !closed;
    }
    int total;
    int at = (int)(c * SCAN_CHUNK) + block_exclusive(n_open, &total, wave_sums);
    if (threadIdx.x == 0) n_open_of[c] = total;
    for (int j = 0; j < 4; ++j)
      if (open[j]) list[at++] = (int)(p0 + j);                     // (at most the chunk's pixels: inside its stretch)
  }
  count_to(status + ST_COMPONENTS, comps);
  count_to(status + ST_SPECKS, specks);
  count_to(status + ST_SPECK_PIXELS, speck_px);
  count_to(status + ST_INVALID_IN, invalid);
}

// ---- the cleanup sweeps ------------------------------------------------------------------------------------------------------
// the end of the stretch of the list that holds chunk c's open pixels (it begins at c SCAN_CHUNK)
__device__ __forceinline__ int64_t open_end(const int32_t* __restrict__ n_open_of, int64_t c, int N) {
  return min(c * SCAN_CHUNK + min(n_open_of[c], SCAN_CHUNK), (int64_t)N);
}

__global__ __launch_bounds__(LABEL_BLOCK) void label_decide_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ list,
                                                                   const int32_t* __restrict__ n_open_of, int32_t* __restrict__ pend,
                                                                   int32_t* __restrict__ words, LabelDims D, int sweep) {
  if (sweep > 0 && words[sweep] == 0) return;                      // the sweep before assigned nothing: nor will this one
  unsigned long long assigned = 0;
  const int64_t chunks = ((int64_t)D.N + SCAN_CHUNK - 1) / SCAN_CHUNK;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t end = open_end(n_open_of, c, D.N);
    for (int64_t i = c * SCAN_CHUNK + threadIdx.x; i < end; i += LABEL_BLOCK) {
      const int p = list[i];
      int choice = -1;
      if ((unsigned)p < (unsigned)D.N && lab[p] < 0) {
        const int x = p % D.nx, y = p / D.nx;
        int v[4];                                                  // left, right, up, down: the root of a closed one, else -1
        v[0] = x > 0 ? lab[p - 1] : D.periodic ? lab[p + D.nx - 1] : -1;
        v[1] = x + 1 < D.nx ? lab[p + 1] : D.periodic ? lab[p - x] : -1;
        v[2] = y > 0 ? lab[p - D.nx] : D.periodic ? lab[(D.ny - 1) * D.nx + x] : -1;
        v[3] = y + 1 < D.ny ? lab[p + D.nx] : D.periodic ? lab[x] : -1;
        int votes = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          if (v[a] < 0) continue;
          int n = 0;
#pragma unroll
          for (int o = 0; o < 4; ++o) n += v[o] == v[a];
          if (n > votes || (n == votes && v[a] < choice)) votes = n, choice = v[a];
        }
        if (choice >= 0) ++assigned;
      }
      pend[i] = choice;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) assigned += __shfl_xor(assigned, m);
  if ((threadIdx.x & 63) == 0 && assigned) atomicAdd(words + 1 + sweep, (int)assigned);
}

__global__ __launch_bounds__(LABEL_BLOCK) void label_commit_kernel(int32_t* __restrict__ lab, const int32_t* __restrict__ list,
                                                                   const int32_t* __restrict__ n_open_of, const int32_t* __restrict__ pend,
                                                                   const int32_t* __restrict__ words, int64_t* __restrict__ status,
                                                                   LabelDims D, int sweep) {
  if (words[1 + sweep] == 0) return;                               // nothing was assigned, or the sweep did not run
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd((unsigned long long*)(status + ST_SWEEPS), 1ull);
  const int64_t chunks = ((int64_t)D.N + SCAN_CHUNK - 1) / SCAN_CHUNK;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t end = open_end(n_open_of, c, D.N);
    for (int64_t i = c * SCAN_CHUNK + threadIdx.x; i < end; i += LABEL_BLOCK) {
      const int choice = pend[i], p = list[i];
      if (choice >= 0 && (unsigned)p < (unsigned)D.N) lab[p] = choice;
    }
  }
}

// ---- rank: an exclusive scan of the grain roots (lab[p] == p), and the output ------------------------------------------------
__device__ __forceinline__ int block_exclusive(int mine, int* total, int* wave_sums) {   // 256 threads, four waves
  int incl = mine;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wave_sums[wave] = incl;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += wave_sums[w];
  *total = wave_sums[0] + wave_sums[1] + wave_sums[2] + wave_sums[3];
  __syncthreads();
  return before + incl - mine;
}

__global__ __launch_bounds__(LABEL_BLOCK) void label_rank_sums_kernel(const int32_t* __restrict__ lab, int32_t* __restrict__ bsum, LabelDims D) {
  __shared__ int wave_sums[4];
  const int64_t p0 = (int64_t)blockIdx.x * SCAN_CHUNK + 4 * threadIdx.x;
  int mine = 0;
  for (int j = 0; j < 4; ++j)
    if (p0 + j < D.N) mine += lab[p0 + j] == (int)(p0 + j);
  int total;
  block_exclusive(mine, &total, wave_sums);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(LABEL_BLOCK) void label_rank_scan_kernel(int32_t* __restrict__ bsum, int64_t chunks, int64_t* __restrict__ status,
                                                                      float* __restrict__ means, int K, int64_t capacity, int noflux) {
  __shared__ int wave_sums[4];
  int carry = 0;
  for (int64_t c0 = 0; c0 < chunks; c0 += LABEL_BLOCK) {            // one workgroup, a carried total
    const int64_t c = c0 + threadIdx.x;
    const int mine = c < chunks ? bsum[c] : 0;
    int total;
    const int before = block_exclusive(mine, &total, wave_sums);
    if (c < chunks) bsum[c] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) {
    status[ST_GRAINS] = carry;
    status[ST_OVERFLOW] = (int64_t)carry + noflux > capacity ? 1 : 0;
  }
  if (noflux && (int)threadIdx.x < K) means[(int64_t)threadIdx.x * capacity] = 0.0f;   // the boundary grain's row
}

__global__ __launch_bounds__(LABEL_BLOCK) void label_rank_add_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ bsum,
                                                                     const uint32_t* __restrict__ size, const long long* __restrict__ sums,
                                                                     int32_t* __restrict__ rank, float* __restrict__ means, LabelDims D,
                                                                     int64_t capacity, int noflux) {
  __shared__ int wave_sums[4];
  const int64_t p0 = (int64_t)blockIdx.x * SCAN_CHUNK + 4 * threadIdx.x;
  bool is_root[4];
  int mine = 0;
  for (int j = 0; j < 4; ++j) {
    is_root[j] = p0 + j < D.N && lab[p0 + j] == (int)(p0 + j);
    mine += is_root[j];
  }
  int total;
  int r = bsum[blockIdx.x] + block_exclusive(mine, &total, wave_sums);
  for (int j = 0; j < 4; ++j) {
    if (!is_root[j]) continue;
    const int64_t p = p0 + j, g = (int64_t)r + noflux;
    rank[p] = r++;
    if (g < capacity)
      for (int k = 0; k < D.K; ++k)
        means[(int64_t)k * capacity + g] = (float)((double)sums[(int64_t)k * D.N + p] / (double)size[p] / 16777216.0);
  }
}

__global__ __launch_bounds__(LABEL_BLOCK) void label_image_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ rank,
                                                                  int32_t* __restrict__ image, int64_t* __restrict__ status, LabelDims D,
                                                                  int first_id) {
  unsigned long long unfilled = 0;
  for (int64_t p = (int64_t)blockIdx.x * LABEL_BLOCK + threadIdx.x; p < D.N; p += (int64_t)gridDim.x * LABEL_BLOCK) {
    const int r = lab[p];
    const bool closed = (unsigned)r < (unsigned)D.N;
    image[p] = closed ? rank[r] + first_id : 0;
    unfilled += !closed;
  }
  count_to(status + ST_UNFILLED, unfilled);
}

// ---- orientations under crystal symmetry (ggnn_label_orientations) ------------------------------------------------------------
// The links byte decided from quaternions, and the per-grain mean quaternion; every stage between is the one above with K = 0.
struct Quat {
  float w, x, y, z;
};
__constant__ float ORIENT_OPS[GGNN_ORIENT_OPS][4] = {
    {1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1},
    {GGNN_ORIENT_H, GGNN_ORIENT_H, 0, 0}, {GGNN_ORIENT_H, -GGNN_ORIENT_H, 0, 0}, {GGNN_ORIENT_H, 0, GGNN_ORIENT_H, 0},
    {GGNN_ORIENT_H, 0, -GGNN_ORIENT_H, 0}, {GGNN_ORIENT_H, 0, 0, GGNN_ORIENT_H}, {GGNN_ORIENT_H, 0, 0, -GGNN_ORIENT_H},
    {0, GGNN_ORIENT_H, GGNN_ORIENT_H, 0}, {0, GGNN_ORIENT_H, -GGNN_ORIENT_H, 0}, {0, GGNN_ORIENT_H, 0, GGNN_ORIENT_H},
    {0, GGNN_ORIENT_H, 0, -GGNN_ORIENT_H}, {0, 0, GGNN_ORIENT_H, GGNN_ORIENT_H}, {0, 0, GGNN_ORIENT_H, -GGNN_ORIENT_H},
    {0.5f, 0.5f, 0.5f, 0.5f}, {0.5f, 0.5f, 0.5f, -0.5f}, {0.5f, 0.5f, -0.5f, 0.5f}, {0.5f, 0.5f, -0.5f, -0.5f},
    {0.5f, -0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f, -0.5f}, {0.5f, -0.5f, -0.5f, 0.5f}, {0.5f, -0.5f, -0.5f, -0.5f}};

__device__ __forceinline__ Quat quat_load(const float* __restrict__ quats, int64_t p, int64_t N) {
  return Quat{quats[p], quats[N + p], quats[2 * N + p], quats[3 * N + p]};
}
__device__ __forceinline__ Quat quat_conj(const Quat& q) { return Quat{q.w, -q.x, -q.y, -q.z}; }
// the header's one product: four products a component, combined left to right, each operation rounded on its own
__device__ __forceinline__ float quat_mul_w(const Quat& p, const Quat& q) {
  return __fsub_rn(__fsub_rn(__fsub_rn(__fmul_rn(p.w, q.w), __fmul_rn(p.x, q.x)), __fmul_rn(p.y, q.y)), __fmul_rn(p.z, q.z));
}
__device__ __forceinline__ Quat quat_mul(const Quat& p, const Quat& q) {
  Quat r;
  r.w = quat_mul_w(p, q);
  r.x = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(p.w, q.x), __fmul_rn(p.x, q.w)), __fmul_rn(p.y, q.z)), __fmul_rn(p.z, q.y));
  r.y = __fadd_rn(__fadd_rn(__fsub_rn(__fmul_rn(p.w, q.y), __fmul_rn(p.x, q.z)), __fmul_rn(p.y, q.w)), __fmul_rn(p.z, q.x));
  r.z = __fadd_rn(__fsub_rn(__fadd_rn(__fmul_rn(p.w, q.z), __fmul_rn(p.x, q.y)), __fmul_rn(p.y, q.x)), __fmul_rn(p.z, q.w));
  return r;
}
__device__ __forceinline__ bool quat_valid(const Quat& q, const uint8_t* __restrict__ mask, int64_t p) {
  if (mask && !mask[p]) return false;
  const float n = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(q.w, q.w), __fmul_rn(q.x, q.x)), __fmul_rn(q.y, q.y)), __fmul_rn(q.z, q.z));
  return fabsf(__fsub_rn(n, 1.0f)) <= 1e-3f;   // (NaN and inf fail the comparison)
}
// cos of half the disorientation of two valid pixels: the largest |w| of r over the group, in closed form
__device__ __forceinline__ float quat_alike(const Quat& a, const Quat& b, bool cubic) {
  const Quat r = quat_mul(quat_conj(a), b);
  if (!cubic) return fabsf(r.w);
  float m1 = fabsf(r.w), m2 = fabsf(r.x), m3 = fabsf(r.y), m4 = fabsf(r.z), t;
#define GGNN_ORDER(hi, lo) t = fmaxf(hi, lo), lo = fminf(hi, lo), hi = t
  GGNN_ORDER(m1, m2);
  GGNN_ORDER(m3, m4);
  GGNN_ORDER(m1, m3);
  GGNN_ORDER(m2, m4);
  GGNN_ORDER(m2, m3);
#undef GGNN_ORDER
  const float s12 = __fadd_rn(m1, m2);
  return fmaxf(m1, fmaxf(__fmul_rn(s12, GGNN_ORIENT_H), __fmul_rn(0.5f, __fadd_rn(s12, __fadd_rn(m3, m4)))));
}

__global__ __launch_bounds__(LABEL_BLOCK) void orient_links_kernel(const float* __restrict__ quats, const uint8_t* __restrict__ mask,
                                                                   uint8_t* __restrict__ links, LabelDims D, float cos_half_tol,
                                                                   bool cubic) {
  const int64_t N = D.N;
  for (int64_t p = (int64_t)blockIdx.x * LABEL_BLOCK + threadIdx.x; p < N; p += (int64_t)gridDim.x * LABEL_BLOCK) {
    uint8_t b = 0;
    const Quat a = quat_load(quats, p, N);
    if (quat_valid(a, mask, p)) {
      b = LINK_VALID;
      const int x = (int)(p % D.nx), y = (int)(p / D.nx);
      if (x + 1 < D.nx || D.periodic) {
        const int64_t q = (int64_t)y * D.nx + (x + 1 < D.nx ? x + 1 : 0);
        const Quat o = quat_load(quats, q, N);
        if (quat_valid(o, mask, q) && quat_alike(a, o, cubic) >= cos_half_tol) b |= LINK_RIGHT;
      }
      if (y + 1 < D.ny || D.periodic) {
        const int64_t q = (int64_t)(y + 1 < D.ny ? y + 1 : 0) * D.nx + x;
        const Quat o = quat_load(quats, q, N);
        if (quat_valid(o, mask, q) && quat_alike(a, o, cubic) >= cos_half_tol) b |= LINK_DOWN;
      }
    }
    links[p] = b;
  }
}

// after classify: lab[p] == p at the roots of the closed components; their four sums, sums[4 root + k], start from 0
__global__ __launch_bounds__(LABEL_BLOCK) void orient_zero_kernel(const int32_t* __restrict__ lab, long long* __restrict__ sums, LabelDims D) {
  for (int64_t p = (int64_t)blockIdx.x * LABEL_BLOCK + threadIdx.x; p < D.N; p += (int64_t)gridDim.x * LABEL_BLOCK)
    if (lab[p] == (int)p)
      for (int k = 0; k < 4; ++k) sums[4 * p + k] = 0;
}

// A thread a pixel, consecutive lanes consecutive raster indices.  A closed pixel (lab >= 0: a pixel of an original component)
// is aligned to its root's equivalent; a wave sums every run of lanes with one root towards the run's first lane -- 64 values
// below 2^24 (1 + 1e-3) fit 32 bits -- and that lane adds the four sums to the root's.  Integers: no order shows in the result.
__global__ __launch_bounds__(LABEL_BLOCK) void orient_accumulate_kernel(const float* __restrict__ quats, const int32_t* __restrict__ lab,
                                                                        long long* sums, LabelDims D, int n_ops) {
  const int lane = threadIdx.x & 63;
  const int64_t N = D.N;
  for (int64_t base = (int64_t)blockIdx.x * LABEL_BLOCK; base < N; base += (int64_t)gridDim.x * LABEL_BLOCK) {   // (uniform in the block)
    const int64_t p = base + threadIdx.x;
    int key = -1, v[4] = {0, 0, 0, 0};
    if (p < N) {
      const int root = lab[p];
      if ((unsigned)root < (unsigned)D.N) {
        key = root;
        const Quat q = quat_load(quats, p, N);
        const Quat r = quat_mul(quat_conj(quat_load(quats, root, N)), q);
        Quat s{ORIENT_OPS[0][0], ORIENT_OPS[0][1], ORIENT_OPS[0][2], ORIENT_OPS[0][3]};
        float c = quat_mul_w(r, s), best = fabsf(c);
        for (int i = 1; i < n_ops; ++i) {
          const Quat si{ORIENT_OPS[i][0], ORIENT_OPS[i][1], ORIENT_OPS[i][2], ORIENT_OPS[i][3]};
          const float ci = quat_mul_w(r, si);
          if (fabsf(ci) > best) best = fabsf(ci), c = ci, s = si;   // (strictly: the first of the largest)
        }
        const Quat a = quat_mul(q, s);
        const float sign = c < 0.0f ? -16777216.0f : 16777216.0f;
        v[0] = (int)__float2ll_rn(__fmul_rn(a.w, sign)), v[1] = (int)__float2ll_rn(__fmul_rn(a.x, sign));
        v[2] = (int)__float2ll_rn(__fmul_rn(a.y, sign)), v[3] = (int)__float2ll_rn(__fmul_rn(a.z, sign));
      }
    }
    const int before = __shfl_up(key, 1);
    const bool head = lane == 0 || before != key;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int end = above ? lane + __ffsll((long long)above) : 64;    // the first lane of the next run
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int o = __shfl_down(v[k], d);
        if (lane + d < end) v[k] += o;
      }
    if (head && key >= 0)
      for (int k = 0; k < 4; ++k) atomicAdd((unsigned long long*)(sums + 4 * (int64_t)key + k), (unsigned long long)(long long)v[k]);
  }
}

// after the rank: the mean of grain root p at row rank[p] (+ 1 with walls, where row 0 is the boundary grain's identity)
__global__ __launch_bounds__(LABEL_BLOCK) void orient_means_kernel(const float* __restrict__ quats, const int32_t* __restrict__ lab,
                                                                   const int32_t* __restrict__ rank, const long long* __restrict__ sums,
                                                                   float* __restrict__ means, LabelDims D, int64_t capacity, int noflux) {
  if (noflux && blockIdx.x == 0 && threadIdx.x < 4) means[(int64_t)threadIdx.x * capacity] = threadIdx.x == 0 ? 1.0f : 0.0f;
  for (int64_t p = (int64_t)blockIdx.x * LABEL_BLOCK + threadIdx.x; p < D.N; p += (int64_t)gridDim.x * LABEL_BLOCK) {
    if (lab[p] != (int)p) continue;
    const int64_t g = (int64_t)rank[p] + noflux;
    if (g >= capacity) continue;
    double d[4];
    for (int k = 0; k < 4; ++k) d[k] = (double)sums[4 * p + k];
    const double n2 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(d[0], d[0]), __dmul_rn(d[1], d[1])), __dmul_rn(d[2], d[2])), __dmul_rn(d[3], d[3]));
    const double len = __dsqrt_rn(n2);
    for (int k = 0; k < 4; ++k) means[(int64_t)k * capacity + g] = n2 == 0.0 ? quats[(int64_t)k * D.N + p] : (float)__ddiv_rn(d[k], len);
  }
}

}  // namespace ggnn

extern "C" size_t ggnn_label_workspace_bytes(int64_t nx, int64_t ny, int32_t K) {
  if (nx < 3 || ny < 3 || nx >= (1 << 15) || ny >= (1 << 15) || K < 0 || K > 4) return 0;
  return ggnn::label_carve(nullptr, nullptr, nx * ny, K);
}

extern "C" int ggnn_label_grains(const ggnn_label_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_label_args& A = *args;
  if ((A.ids != nullptr) == (A.angles != nullptr) || !A.image || !A.status || !A.workspace) return GGNN_EINVAL;
  if (A.nx < 3 || A.ny < 3 || A.nx >= (1 << 15) || A.ny >= (1 << 15)) return GGNN_EINVAL;
  if (A.angles ? A.K < 1 || A.K > 4 || !A.mean_angles || !(A.tol >= 0.0f) : A.K != 0) return GGNN_EINVAL;
  if (A.min_pixels < 1 || A.max_sweeps < 0 || A.max_sweeps > GGNN_LABEL_MAX_SWEEPS) return GGNN_EINVAL;
  if (A.grain_capacity < 1 || A.grain_capacity >= INT32_MAX) return GGNN_EINVAL;
  if (A.boundary != GGNN_BC_PERIODIC && A.boundary != GGNN_BC_NOFLUX) return GGNN_EINVAL;
  if ((reinterpret_cast<uintptr_t>(A.status) & 7u) || (reinterpret_cast<uintptr_t>(A.workspace) & 7u) ||
      (reinterpret_cast<uintptr_t>(A.image) & 3u) || (reinterpret_cast<uintptr_t>(A.ids) & 3u) ||
      (reinterpret_cast<uintptr_t>(A.angles) & 3u) || (reinterpret_cast<uintptr_t>(A.mean_angles) & 3u))
    return GGNN_EINVAL;
  const int64_t N = A.nx * A.ny;
  LabelWs W;
  if (A.workspace_bytes < label_carve(&W, (char*)A.workspace, N, A.K)) return GGNN_EINVAL;
  const LabelDims D{(int)A.nx, (int)A.ny, (int)N, A.K, A.boundary == GGNN_BC_PERIODIC};
  const int noflux = D.periodic ? 0 : 1;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(A.status, 0, GGNN_LABEL_STATUS_WORDS * sizeof(int64_t), st) != hipSuccess) return GGNN_ELAUNCH;
  if (hipMemsetAsync(W.words, 0, label_words_bytes(), st) != hipSuccess) return GGNN_ELAUNCH;
  const int64_t wide = std::min<int64_t>((N + LABEL_BLOCK - 1) / LABEL_BLOCK, 16 * (int64_t)num_cu());   // grid-stride passes
  const dim3 pass((unsigned)wide), block(LABEL_BLOCK);
  if (A.angles)
    hipLaunchKernelGGL(label_links_kernel<true>, pass, block, 0, st, A.ids, A.angles, A.valid, W.links, D, A.tol);
  else
    hipLaunchKernelGGL(label_links_kernel<false>, pass, block, 0, st, A.ids, A.angles, A.valid, W.links, D, A.tol);
  const int tiles_x = (D.nx + LABEL_TX - 1) / LABEL_TX, tiles_y = (D.ny + LABEL_TY - 1) / LABEL_TY;
  const size_t lds = (size_t)LABEL_TILE * (8 + 8 * (size_t)A.K);
  hipLaunchKernelGGL(label_tile_kernel, dim3((unsigned)(tiles_x * tiles_y)), block, lds, st, A.angles, W.links, W.parent, W.size,
                     W.sums, A.status, D, tiles_x);
  const int64_t seams = (int64_t)D.ny * tiles_x + (int64_t)D.nx * tiles_y;
  hipLaunchKernelGGL(label_seam_kernel, dim3((unsigned)std::min<int64_t>((seams + LABEL_BLOCK - 1) / LABEL_BLOCK, wide)), block, 0, st,
                     W.links, W.parent, A.status, D, tiles_x, tiles_y);
  hipLaunchKernelGGL(label_flatten_kernel, pass, block, 0, st, W.links, W.parent, W.size, W.sums, W.lab, A.status, D);
  hipLaunchKernelGGL(label_classify_kernel, pass, block, 0, st, W.links, W.size, W.lab, W.list, W.open, A.status, D, A.min_pixels);
  int32_t* pend = W.parent;                                       // (the parents are dead: every root is in lab)
  const dim3 few((unsigned)std::min<int64_t>(wide, 2 * (int64_t)num_cu()));   // (most sweeps return at once: a small grid strides the list)
  for (int s = 0; s < A.max_sweeps; ++s) {
    hipLaunchKernelGGL(label_decide_kernel, few, block, 0, st, W.lab, W.list, W.open, pend, W.words, D, s);
    hipLaunchKernelGGL(label_commit_kernel, few, block, 0, st, W.lab, W.list, W.open, pend, W.words, A.status, D, s);
  }
  const int64_t chunks = (N + SCAN_CHUNK - 1) / SCAN_CHUNK;
  hipLaunchKernelGGL(label_rank_sums_kernel, dim3((unsigned)chunks), block, 0, st, W.lab, W.bsum, D);
  hipLaunchKernelGGL(label_rank_scan_kernel, dim3(1), block, 0, st, W.bsum, chunks, A.status, A.mean_angles, A.K, A.grain_capacity, noflux);
  hipLaunchKernelGGL(label_rank_add_kernel, dim3((unsigned)chunks), block, 0, st, W.lab, W.bsum, W.size, W.sums, W.rank, A.mean_angles, D,
                     A.grain_capacity, noflux);
  hipLaunchKernelGGL(label_image_kernel, pass, block, 0, st, W.lab, W.rank, A.image, A.status, D, D.periodic ? 1 : 2);
  return launch_status();
}

extern "C" size_t ggnn_label_orient_workspace_bytes(int64_t nx, int64_t ny) {
  if (nx < 3 || ny < 3 || nx >= (1 << 15) || ny >= (1 << 15)) return 0;
  return ggnn::label_carve(nullptr, nullptr, nx * ny, 4);
}

extern "C" int ggnn_label_orientations(const ggnn_label_orient_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_label_orient_args& A = *args;
  if (!A.quats || !A.image || !A.mean_quats || !A.status || !A.workspace) return GGNN_EINVAL;
  if (A.nx < 3 || A.ny < 3 || A.nx >= (1 << 15) || A.ny >= (1 << 15)) return GGNN_EINVAL;
  if (!(A.cos_half_tol > GGNN_ORIENT_H && A.cos_half_tol <= 1.0f)) return GGNN_EINVAL;
  if (A.symmetry != GGNN_SYM_NONE && A.symmetry != GGNN_SYM_CUBIC) return GGNN_EINVAL;
  if (A.min_pixels < 1 || A.max_sweeps < 0 || A.max_sweeps > GGNN_LABEL_MAX_SWEEPS) return GGNN_EINVAL;
  if (A.grain_capacity < 1 || A.grain_capacity >= INT32_MAX) return GGNN_EINVAL;
  if (A.boundary != GGNN_BC_PERIODIC && A.boundary != GGNN_BC_NOFLUX) return GGNN_EINVAL;
  if ((reinterpret_cast<uintptr_t>(A.status) & 7u) || (reinterpret_cast<uintptr_t>(A.workspace) & 7u) ||
      (reinterpret_cast<uintptr_t>(A.image) & 3u) || (reinterpret_cast<uintptr_t>(A.quats) & 3u) ||
      (reinterpret_cast<uintptr_t>(A.mean_quats) & 3u))
    return GGNN_EINVAL;
  const int64_t N = A.nx * A.ny;
  LabelWs W;
  if (A.workspace_bytes < label_carve(&W, (char*)A.workspace, N, 4)) return GGNN_EINVAL;
  const LabelDims D{(int)A.nx, (int)A.ny, (int)N, 0, A.boundary == GGNN_BC_PERIODIC};   // K = 0: the stages carry no angle sums
  const int noflux = D.periodic ? 0 : 1;
  const bool cubic = A.symmetry == GGNN_SYM_CUBIC;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(A.status, 0, GGNN_LABEL_STATUS_WORDS * sizeof(int64_t), st) != hipSuccess) return GGNN_ELAUNCH;
  if (hipMemsetAsync(W.words, 0, label_words_bytes(), st) != hipSuccess) return GGNN_ELAUNCH;
  const int64_t wide = std::min<int64_t>((N + LABEL_BLOCK - 1) / LABEL_BLOCK, 16 * (int64_t)num_cu());
  const dim3 pass((unsigned)wide), block(LABEL_BLOCK);
  hipLaunchKernelGGL(orient_links_kernel, pass, block, 0, st, A.quats, A.valid, W.links, D, A.cos_half_tol, cubic);
  const int tiles_x = (D.nx + LABEL_TX - 1) / LABEL_TX, tiles_y = (D.ny + LABEL_TY - 1) / LABEL_TY;
  hipLaunchKernelGGL(label_tile_kernel, dim3((unsigned)(tiles_x * tiles_y)), block, (size_t)LABEL_TILE * 8, st, (const float*)nullptr,
                     W.links, W.parent, W.size, W.sums, A.status, D, tiles_x);
  const int64_t seams = (int64_t)D.ny * tiles_x + (int64_t)D.nx * tiles_y;
  hipLaunchKernelGGL(label_seam_kernel, dim3((unsigned)std::min<int64_t>((seams + LABEL_BLOCK - 1) / LABEL_BLOCK, wide)), block, 0, st,
                     W.links, W.parent, A.status, D, tiles_x, tiles_y);
  hipLaunchKernelGGL(label_flatten_kernel, pass, block, 0, st, W.links, W.parent, W.size, W.sums, W.lab, A.status, D);
  hipLaunchKernelGGL(label_classify_kernel, pass, block, 0, st, W.links, W.size, W.lab, W.list, W.open, A.status, D, A.min_pixels);
  hipLaunchKernelGGL(orient_zero_kernel, pass, block, 0, st, W.lab, W.sums, D);      // (lab still marks the open pixels with -1)
  hipLaunchKernelGGL(orient_accumulate_kernel, pass, block, 0, st, A.quats, W.lab, W.sums, D, cubic ? GGNN_ORIENT_OPS : 1);
  int32_t* pend = W.parent;
  const dim3 few((unsigned)std::min<int64_t>(wide, 2 * (int64_t)num_cu()));
  for (int s = 0; s < A.max_sweeps; ++s) {
    hipLaunchKernelGGL(label_decide_kernel, few, block, 0, st, W.lab, W.list, W.open, pend, W.words, D, s);
    hipLaunchKernelGGL(label_commit_kernel, few, block, 0, st, W.lab, W.list, W.open, pend, W.words, A.status, D, s);
  }
  const int64_t chunks = (N + SCAN_CHUNK - 1) / SCAN_CHUNK;
  hipLaunchKernelGGL(label_rank_sums_kernel, dim3((unsigned)chunks), block, 0, st, W.lab, W.bsum, D);
  hipLaunchKernelGGL(label_rank_scan_kernel, dim3(1), block, 0, st, W.bsum, chunks, A.status, (float*)nullptr, 0, A.grain_capacity, noflux);
  hipLaunchKernelGGL(label_rank_add_kernel, dim3((unsigned)chunks), block, 0, st, W.lab, W.bsum, W.size, W.sums, W.rank, (float*)nullptr, D,
                     A.grain_capacity, noflux);
  hipLaunchKernelGGL(orient_means_kernel, pass, block, 0, st, A.quats, W.lab, W.rank, W.sums, A.mean_quats, D, A.grain_capacity, noflux);
  hipLaunchKernelGGL(label_image_kernel, pass, block, 0, st, W.lab, W.rank, A.image, A.status, D, D.periodic ? 1 : 2);
  return launch_status();
}
