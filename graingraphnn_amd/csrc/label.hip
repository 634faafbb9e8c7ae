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
// A STACK of T equal-shaped maps (ggnn_label_grains_stack, ggnn_label_orientations_stack) runs the same launches: every stage
// has a frame dimension, and one map is the stack with T = 1 (one host routine, label_run, behind all four entry points).  Pixel p
// of frame t is the index t N + p of every per-pixel array, N = ny nx, and T N fits int32.  Frames never meet: a tile, a seam, a
// neighbour and a wrap stay inside one frame; a chunk of SCAN_CHUNK pixels never straddles two (ceil(N / SCAN_CHUNK) chunks a
// frame, the last one partial); every frame has its own status row, its own sweep words and its own rank.  What a frame gets
// is, bit for bit, what the single call gives on it.
//
// No kernel waits on another workgroup: the order between workgroups is the order of the launches.  Every loop that follows
// parents carries a budget of hops derived from the number of pixels OF ONE FRAME; a thread that spends it counts itself in
// its frame's n_bound_hits and leaves.  Parent words that another workgroup may write in the same launch (the seam merge) are
// read and written with agent-scope atomics alone.
#include <algorithm>

#include "common.h"

namespace ggnn {

constexpr int LABEL_TX = GGNN_LABEL_TILE_X, LABEL_TY = GGNN_LABEL_TILE_Y;
constexpr int LABEL_TILE = LABEL_TX * LABEL_TY;          // 1024 pixels: 256 threads, four neighbouring pixels each
constexpr int LABEL_BLOCK = 256;
constexpr int LABEL_PER_THREAD = LABEL_TILE / LABEL_BLOCK;
constexpr int SCAN_CHUNK = 4 * LABEL_BLOCK;
constexpr int LABEL_SWEEP_WORDS = GGNN_LABEL_MAX_SWEEPS + 1;
constexpr uint8_t LINK_RIGHT = 1, LINK_DOWN = 2, LINK_VALID = 4, LINK_LOCAL_ROOT = 8;
enum { ST_COMPONENTS, ST_SPECKS, ST_SPECK_PIXELS, ST_INVALID_IN, ST_GRAINS, ST_SWEEPS, ST_UNFILLED, ST_OVERFLOW, ST_BOUND_HITS };
static_assert(LABEL_TX % LABEL_PER_THREAD == 0 && LABEL_TILE % LABEL_BLOCK == 0, "a thread's pixels lie in one row of the tile");
static_assert(ST_BOUND_HITS + 1 == GGNN_LABEL_STATUS_WORDS, "the status words of include/ggnn.h");

struct LabelWs {          // the carved workspace; n = T N pixels, chunk c of frame t is chunk t chunks + c
  int32_t* words;         // [T, 1 + max_sweeps]: [t][1 + s] the pixels sweep s assigned in frame t ([t][0] spare); with T > 1 one
                          // more row, the sums over the frames (with one frame, the frame's row is that row)
  uint8_t* links;         // [n]
  int32_t* parent;        // [n]; dead after flatten: the sweeps' side array lives here
  uint32_t* size;         // [n], at roots
  int32_t* lab;           // [n]: the root of a closed pixel, -1 open
  int32_t* list;          // [n]: the open pixels of chunk c of frame t at t N + c SCAN_CHUNK .. + open[t chunks + c]
  int32_t* open;          // [T chunks]
  int32_t* rank;          // [n], at grain roots: the rank within the frame
  int32_t* bsum;          // [T chunks]
  long long* sums;        // [K, n], at roots (orientations: [n, 4])
};
constexpr size_t LABEL_ALIGN = 256;
static inline size_t up(size_t b) { return (b + LABEL_ALIGN - 1) / LABEL_ALIGN * LABEL_ALIGN; }
static inline size_t label_word_rows(int64_t T) { return (size_t)T + (T > 1 ? 1 : 0); }
static size_t label_carve(LabelWs* w, char* base, int64_t T, int64_t N, int K) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += up(bytes);
    return p;
  };
  const size_t n = (size_t)T * (size_t)N, chunks = (size_t)T * (((size_t)N + SCAN_CHUNK - 1) / SCAN_CHUNK);
  char* words = take(label_word_rows(T) * LABEL_SWEEP_WORDS * sizeof(int32_t));
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
  int nx, ny, N, K;       // one frame: N = nx ny pixels, K angle channels
  int T, NT, chunks;      // T frames, NT = T N pixels in all (it fits int32), chunks of SCAN_CHUNK pixels a frame
  int wstride;            // 1 + max_sweeps: a frame's row of sweep words
  bool periodic;
};

// the frame of pixel (or list position) p of the stack
__device__ __forceinline__ int frame_of(int64_t p, const LabelDims& D) { return D.T == 1 ? 0 : (int)((unsigned)p / (unsigned)D.N); }

// v added to word `word` of frame `frame`'s status row.  Whole waves call it.  In a pass over all T N pixels the lanes of a wave
// lie in different frames as soon as N is no multiple of 64 (at 3 x 3 seven frames share a wave): a sum over the wave and one
// atomic where all lanes name one frame, an atomic a lane where they do not.
__device__ __forceinline__ void count_to(int64_t* status, int frame, int word, unsigned long long v) {
  int64_t* at = status + (int64_t)frame * GGNN_LABEL_STATUS_WORDS + word;
  if (__all(frame == __shfl(frame, 0))) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long*)at, v);
  } else if (v) {
    atomicAdd((unsigned long long*)at, v);
  }
}
// a thread that spent the budget of a parent walk (never, unless a bound is wrong: no reduction)
__device__ __forceinline__ void count_hit(int64_t* status, int frame) {
  atomicAdd((unsigned long long*)(status + (int64_t)frame * GGNN_LABEL_STATUS_WORDS + ST_BOUND_HITS), 1ull);
}
// A thread's count over a pass whose pixels run through the frames in order: it belongs to the frame the thread is in, and goes
// to that frame's row when any lane of the wave moves on to another frame (whole waves call enter; with T = 1 nobody moves).
struct FrameCount {
  int frame;
  unsigned long long v;
  __device__ __forceinline__ void enter(int64_t* status, int word, int f) {
    if (__any(f != frame)) {
      count_to(status, frame, word, v);
      frame = f, v = 0;
    }
  }
};

// ---- links -------------------------------------------------------------------------------------------------------------------
// (ids, angles and mask: one frame's; p, q: pixels of the frame)
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
__global__ __launch_bounds__(LABEL_BLOCK) void label_links_kernel(const int32_t* __restrict__ all_ids, const float* __restrict__ all_angles,
                                                                  const uint8_t* __restrict__ all_mask, uint8_t* __restrict__ links,
                                                                  LabelDims D, float tol) {
  const int64_t N = D.N;
  for (int64_t g = (int64_t)blockIdx.x * LABEL_BLOCK + threadIdx.x; g < D.NT; g += (int64_t)gridDim.x * LABEL_BLOCK) {
    const int64_t f = frame_of(g, D), p = g - f * N;
    const int32_t* ids = ANGLES ? nullptr : all_ids + f * N;
    const float* angles = ANGLES ? all_angles + f * D.K * N : nullptr;
    const uint8_t* mask = all_mask ? all_mask + f * N : nullptr;
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
    links[g] = b;
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

// workgroup b: tile b % tiles of frame b / tiles
__global__ __launch_bounds__(LABEL_BLOCK) void label_tile_kernel(const float* __restrict__ all_angles, uint8_t* __restrict__ all_links,
                                                                 int32_t* __restrict__ all_parent, uint32_t* __restrict__ all_size,
                                                                 long long* __restrict__ all_sums, int64_t* __restrict__ status,
                                                                 LabelDims D, int tiles_x, int tiles) {
  extern __shared__ long long label_lds[];                       // [K][LABEL_TILE] sums, then the labels and the counts
  long long* lsum = label_lds;
  int* lab = (int*)(label_lds + (size_t)D.K * LABEL_TILE);
  unsigned* cnt = (unsigned*)(lab + LABEL_TILE);
  const int frame = blockIdx.x / tiles, tile = blockIdx.x - frame * tiles;
  const int64_t at = (int64_t)frame * D.N;                        // the frame's first pixel
  const float* angles = all_angles ? all_angles + at * D.K : nullptr;
  uint8_t* links = all_links + at;
  int32_t* parent = all_parent + at;
  uint32_t* size = all_size + at;
  long long* sums = all_sums + at;                               // (channel k of pixel p of the stack at k NT + p)
  const int x0 = (tile % tiles_x) * LABEL_TX, y0 = (tile / tiles_x) * LABEL_TY;
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
    parent[p] = (int)at + (y0 + r / LABEL_TX) * D.nx + x0 + r % LABEL_TX;   // (a root lies inside the image: it is a pixel of it)
    if (r == i) {
      size[p] = cnt[i];
      for (int k = 0; k < D.K; ++k) sums[(int64_t)k * D.NT + p] = lsum[k * LABEL_TILE + i];
      if (b[j] & LINK_VALID) links[p] = b[j] | LINK_LOCAL_ROOT;
    }
  }
  count_to(status, frame, ST_BOUND_HITS, hits);                  // (a workgroup lies in one frame)
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
  // the pairs of a frame: (right) ny rows x tiles_x last columns, then (down) nx columns x tiles_y last rows; frame after frame
  const int64_t n_right = (int64_t)D.ny * tiles_x, n_frame = n_right + (int64_t)D.nx * tiles_y, n_all = n_frame * D.T;
  for (int64_t g = (int64_t)blockIdx.x * LABEL_BLOCK + threadIdx.x; g < n_all; g += (int64_t)gridDim.x * LABEL_BLOCK) {
    const int frame = D.T == 1 ? 0 : (int)(g / n_frame);
    const int64_t t = g - frame * n_frame;
    const int at = frame * D.N;
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
    if (!(links[at + (int64_t)y * D.nx + x] & want)) continue;
    int a = at + y * D.nx + x, b = at + y2 * D.nx + x2;         // (the wrap goes to the frame's own row 0 or column 0)
    int64_t budget = 2 * (int64_t)D.N + 64;                       // hops of this union, its retries included: one frame's pixels
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
    if (!done) count_hit(status, frame);
  }
}

// ---- flatten, classify -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LABEL_BLOCK) void label_flatten_kernel(const uint8_t* __restrict__ links, const int32_t* __restrict__ parent,
                                                                    uint32_t* size, long long* sums, int32_t* __restrict__ lab,
                                                                    int64_t* __restrict__ status, LabelDims D) {
  for (int64_t p = (int64_t)blockIdx.x * LABEL_BLOCK + threadIdx.x; p < D.NT; p += (int64_t)gridDim.x * LABEL_BLOCK) {
    int x = (int)p;
    int64_t budget = (int64_t)D.N + 1;                             // (a chain stays inside its frame)
    bool found = false;
    while (budget-- > 0) {                                         // (parents are not written in this launch: plain loads)
      const int up = parent[x];
      if (up == x) {
        found = true;
        break;
      }
      x = up;
    }
    if (!found) x = (int)p, count_hit(status, frame_of(p, D));
    lab[p] = x;
    if ((links[p] & LINK_LOCAL_ROOT) && x != (int)p) {             // a tile-local component joins its root: one atomic each
      atomicAdd(size + x, size[p]);
      for (int k = 0; k < D.K; ++k)
        atomicAdd((unsigned long long*)(sums + (int64_t)k * D.NT + x), (unsigned long long)sums[(int64_t)k * D.NT + p]);
    }
  }
}

__device__ __forceinline__ int block_exclusive(int mine, int* total, int* wave_sums);

// A workgroup takes chunks of SCAN_CHUNK pixels, four neighbouring ones a thread, and lists a chunk's open pixels in the chunk's
// own stretch of the list, with their number beside it: no counter is shared between workgroups (one atomic a wave of 64 pixels
// on a shared counter cost 0.76 ms of this pass's 1.57 ms at 4 096 x 4 096 with 1 % noise; the 0.81 ms left are not the list's:
// DESIGN 8o).  A chunk lies in one frame, so a workgroup's counts are one frame's until its chunks move on to the next.
__global__ __launch_bounds__(LABEL_BLOCK) void label_classify_kernel(const uint8_t* __restrict__ links, const uint32_t* __restrict__ size,
                                                                     int32_t* __restrict__ lab, int32_t* __restrict__ list,
                                                                     int32_t* __restrict__ n_open_of, int64_t* __restrict__ status,
                                                                     LabelDims D, int64_t min_pixels) {
  __shared__ int wave_sums[4];
  unsigned long long comps = 0, specks = 0, speck_px = 0, invalid = 0;
  const int64_t chunks = (int64_t)D.T * D.chunks;
  int frame = -1;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int f = D.T == 1 ? 0 : (int)(c / D.chunks);
    if (f != frame) {                                              // (uniform in the workgroup)
      if (frame >= 0) {
        count_to(status, frame, ST_COMPONENTS, comps), count_to(status, frame, ST_SPECKS, specks);
        count_to(status, frame, ST_SPECK_PIXELS, speck_px), count_to(status, frame, ST_INVALID_IN, invalid);
      }
      frame = f, comps = specks = speck_px = invalid = 0;
    }
    const int64_t at = (int64_t)f * D.N, end = at + D.N;           // the frame's pixels
    const int64_t c0 = at + (c - (int64_t)f * D.chunks) * SCAN_CHUNK, p0 = c0 + 4 * threadIdx.x;
    bool open[4];
    int n_open = 0;
    for (int j = 0; j < 4; ++j) {
      const int64_t p = p0 + j;
      open[j] = false;
      if (p >= end) continue;
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
    int64_t to = c0 + block_exclusive(n_open, &total, wave_sums);
    if (threadIdx.x == 0) n_open_of[c] = total;
    for (int j = 0; j < 4; ++j)
      if (open[j]) list[to++] = (int)(p0 + j);                     // (at most the chunk's pixels: inside its stretch)
  }
  if (frame >= 0) {
    count_to(status, frame, ST_COMPONENTS, comps), count_to(status, frame, ST_SPECKS, specks);
    count_to(status, frame, ST_SPECK_PIXELS, speck_px), count_to(status, frame, ST_INVALID_IN, invalid);
  }
}

// ---- the cleanup sweeps ------------------------------------------------------------------------------------------------------
// Frame t's row of sweep words is words + t wstride.  The row of the sums over the frames, by which a launch knows that every
// frame has gone quiet, follows the T rows; with one frame the frame's row is that row.
__device__ __forceinline__ const int32_t* any_words(const int32_t* words, const LabelDims& D) {
  return D.T == 1 ? words : words + (int64_t)D.T * D.wstride;
}
// the stretch of the list that holds the open pixels of chunk c (of the stack), which lies in frame f
__device__ __forceinline__ void open_stretch(const int32_t* __restrict__ n_open_of, int64_t c, int f, const LabelDims& D, int64_t* begin,
                                             int64_t* end) {
  const int64_t at = (int64_t)f * D.N;
  *begin = at + (c - (int64_t)f * D.chunks) * SCAN_CHUNK;
  *end = min(*begin + min(n_open_of[c], SCAN_CHUNK), at + D.N);
}

__global__ __launch_bounds__(LABEL_BLOCK) void label_decide_kernel(const int32_t* __restrict__ all_lab, const int32_t* __restrict__ list,
                                                                   const int32_t* __restrict__ n_open_of, int32_t* __restrict__ pend,
                                                                   int32_t* __restrict__ words, LabelDims D, int sweep) {
  if (sweep > 0 && any_words(words, D)[sweep] == 0) return;        // the sweep before assigned nothing in any frame: nor will this one
  int assigned = 0, frame = -1;
  auto hand_over = [&]() {                                         // the workgroup's count to its frame's word, and to the sum
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) assigned += __shfl_xor(assigned, m);
    if ((threadIdx.x & 63) == 0 && assigned) {
      atomicAdd(words + (int64_t)frame * D.wstride + 1 + sweep, assigned);
      if (D.T > 1) atomicAdd(words + (int64_t)D.T * D.wstride + 1 + sweep, assigned);
    }
  };
  const int64_t chunks = (int64_t)D.T * D.chunks;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int f = D.T == 1 ? 0 : (int)(c / D.chunks);
    if (f != frame) {                                              // (uniform in the workgroup)
      if (frame >= 0) hand_over();
      frame = f, assigned = 0;
    }
    if (sweep > 0 && words[(int64_t)f * D.wstride + sweep] == 0) continue;   // this frame has gone quiet
    const int32_t* lab = all_lab + (int64_t)f * D.N;              // the frame's: neighbours and wraps stay inside it
    int64_t begin, end;
    open_stretch(n_open_of, c, f, D, &begin, &end);
    for (int64_t i = begin + threadIdx.x; i < end; i += LABEL_BLOCK) {
      const int p = list[i] - f * D.N;
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
  if (frame >= 0) hand_over();
}

__global__ __launch_bounds__(LABEL_BLOCK) void label_commit_kernel(int32_t* __restrict__ lab, const int32_t* __restrict__ list,
                                                                   const int32_t* __restrict__ n_open_of, const int32_t* __restrict__ pend,
                                                                   const int32_t* __restrict__ words, int64_t* __restrict__ status,
                                                                   LabelDims D, int sweep) {
  if (any_words(words, D)[1 + sweep] == 0) return;                 // nothing was assigned in any frame, or the sweep did not run
  const int64_t chunks = (int64_t)D.T * D.chunks;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int f = D.T == 1 ? 0 : (int)(c / D.chunks);
    if (words[(int64_t)f * D.wstride + 1 + sweep] == 0) continue;  // nothing was assigned in this frame
    if (c == (int64_t)f * D.chunks && threadIdx.x == 0)            // (the frame's first chunk: once a frame)
      atomicAdd((unsigned long long*)(status + (int64_t)f * GGNN_LABEL_STATUS_WORDS + ST_SWEEPS), 1ull);
    int64_t begin, end;
    open_stretch(n_open_of, c, f, D, &begin, &end);
    for (int64_t i = begin + threadIdx.x; i < end; i += LABEL_BLOCK) {
      const int choice = pend[i], p = list[i];
      if (choice >= 0 && (unsigned)(p - f * D.N) < (unsigned)D.N) lab[p] = choice;
    }
  }
}

// ---- rank: an exclusive scan of the grain roots (lab[p] == p) of every frame, and the output -----------------------------------
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

// workgroup b: chunk b % chunks of frame b / chunks -> the chunk's first pixel and the end of its frame
__device__ __forceinline__ int64_t chunk_pixels(const LabelDims& D, int* frame, int64_t* end) {
  *frame = blockIdx.x / D.chunks;
  const int64_t at = (int64_t)*frame * D.N;
  *end = at + D.N;
  return at + (int64_t)(blockIdx.x - *frame * D.chunks) * SCAN_CHUNK;
}

__global__ __launch_bounds__(LABEL_BLOCK) void label_rank_sums_kernel(const int32_t* __restrict__ lab, int32_t* __restrict__ bsum, LabelDims D) {
  __shared__ int wave_sums[4];
  int frame;
  int64_t end;
  const int64_t p0 = chunk_pixels(D, &frame, &end) + 4 * threadIdx.x;
  int mine = 0;
  for (int j = 0; j < 4; ++j)
    if (p0 + j < end) mine += lab[p0 + j] == (int)(p0 + j);
  int total;
  block_exclusive(mine, &total, wave_sums);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup a frame: the frame's block sums, its n_grains and overflow, the boundary grain's row of its means
__global__ __launch_bounds__(LABEL_BLOCK) void label_rank_scan_kernel(int32_t* __restrict__ all_bsum, int64_t chunks, int64_t* __restrict__ all_status,
                                                                      float* __restrict__ all_means, int K, int64_t capacity, int noflux) {
  __shared__ int wave_sums[4];
  int32_t* bsum = all_bsum + (int64_t)blockIdx.x * chunks;
  int64_t* status = all_status + (int64_t)blockIdx.x * GGNN_LABEL_STATUS_WORDS;
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
  if (noflux && (int)threadIdx.x < K) all_means[((int64_t)blockIdx.x * K + threadIdx.x) * capacity] = 0.0f;   // the boundary grain's row
}

__global__ __launch_bounds__(LABEL_BLOCK) void label_rank_add_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ bsum,
                                                                     const uint32_t* __restrict__ size, const long long* __restrict__ sums,
                                                                     int32_t* __restrict__ rank, float* __restrict__ all_means, LabelDims D,
                                                                     int64_t capacity, int noflux) {
  __shared__ int wave_sums[4];
  int frame;
  int64_t end;
  const int64_t p0 = chunk_pixels(D, &frame, &end) + 4 * threadIdx.x;
  float* means = all_means + (int64_t)frame * D.K * capacity;      // (not addressed with K = 0)
  bool is_root[4];
  int mine = 0;
  for (int j = 0; j < 4; ++j) {
    is_root[j] = p0 + j < end && lab[p0 + j] == (int)(p0 + j);
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
        means[(int64_t)k * capacity + g] = (float)((double)sums[(int64_t)k * D.NT + p] / (double)size[p] / 16777216.0);
  }
}

// Whole waves walk the pixels (a lane past the end holds nothing and stands in the last frame), so that FrameCount may shuffle.
__global__ __launch_bounds__(LABEL_BLOCK) void label_image_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ rank,
                                                                  int32_t* __restrict__ image, int64_t* __restrict__ status, LabelDims D,
                                                                  int first_id) {
  const int64_t last = (int64_t)D.NT - 1;
  FrameCount unfilled{frame_of(min((int64_t)blockIdx.x * LABEL_BLOCK + threadIdx.x, last), D), 0};
  for (int64_t base = (int64_t)blockIdx.x * LABEL_BLOCK; base < D.NT; base += (int64_t)gridDim.x * LABEL_BLOCK) {   // (uniform in the block)
    const int64_t p = base + threadIdx.x;
    unfilled.enter(status, ST_UNFILLED, frame_of(min(p, last), D));
    if (p <= last) {
      const int r = lab[p];
      const bool closed = (unsigned)r < (unsigned)D.NT;           // (a root lies in the pixel's own frame)
      image[p] = closed ? rank[r] + first_id : 0;
      unfilled.v += !closed;
    }
  }
  count_to(status, unfilled.frame, ST_UNFILLED, unfilled.v);
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

// (quats: one frame's four planes; p: a pixel of the frame)
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

__global__ __launch_bounds__(LABEL_BLOCK) void orient_links_kernel(const float* __restrict__ all_quats, const uint8_t* __restrict__ all_mask,
                                                                   uint8_t* __restrict__ links, LabelDims D, float cos_half_tol,
                                                                   bool cubic) {
  const int64_t N = D.N;
  for (int64_t g = (int64_t)blockIdx.x * LABEL_BLOCK + threadIdx.x; g < D.NT; g += (int64_t)gridDim.x * LABEL_BLOCK) {
    const int64_t f = frame_of(g, D), p = g - f * N;
    const float* quats = all_quats + 4 * f * N;
    const uint8_t* mask = all_mask ? all_mask + f * N : nullptr;
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
    links[g] = b;
  }
}

// after classify: lab[p] == p at the roots of the closed components; their four sums, sums[4 root + k], start from 0
__global__ __launch_bounds__(LABEL_BLOCK) void orient_zero_kernel(const int32_t* __restrict__ lab, long long* __restrict__ sums, LabelDims D) {
  for (int64_t p = (int64_t)blockIdx.x * LABEL_BLOCK + threadIdx.x; p < D.NT; p += (int64_t)gridDim.x * LABEL_BLOCK)
    if (lab[p] == (int)p)
      for (int k = 0; k < 4; ++k) sums[4 * p + k] = 0;
}

// A thread a pixel, consecutive lanes consecutive raster indices.  A closed pixel (lab >= 0: a pixel of an original component)
// is aligned to its root's equivalent; a wave sums every run of lanes with one root towards the run's first lane -- 64 values
// below 2^24 (1 + 1e-3) fit 32 bits -- and that lane adds the four sums to the root's.  Integers: no order shows in the result.
// (A root names one frame's component: a run never crosses a frame.)
__global__ __launch_bounds__(LABEL_BLOCK) void orient_accumulate_kernel(const float* __restrict__ all_quats, const int32_t* __restrict__ lab,
                                                                        long long* sums, LabelDims D, int n_ops) {
  const int lane = threadIdx.x & 63;
  const int64_t N = D.N;
  for (int64_t base = (int64_t)blockIdx.x * LABEL_BLOCK; base < D.NT; base += (int64_t)gridDim.x * LABEL_BLOCK) {   // (uniform in the block)
    const int64_t p = base + threadIdx.x;
    int key = -1, v[4] = {0, 0, 0, 0};
    if (p < D.NT) {
      const int root = lab[p];
      if ((unsigned)root < (unsigned)D.NT) {
        key = root;
        const int64_t at = (int64_t)frame_of(p, D) * N;           // the frame of the pixel and of its root
        const float* quats = all_quats + 4 * at;
        const Quat q = quat_load(quats, p - at, N);
        const Quat r = quat_mul(quat_conj(quat_load(quats, root - at, N)), q);
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

// after the rank: the mean of grain root p at row rank[p] of its frame (+ 1 with walls, where row 0 is the boundary grain's identity)
__global__ __launch_bounds__(LABEL_BLOCK) void orient_means_kernel(const float* __restrict__ quats, const int32_t* __restrict__ lab,
                                                                   const int32_t* __restrict__ rank, const long long* __restrict__ sums,
                                                                   float* __restrict__ means, LabelDims D, int64_t capacity, int noflux) {
  if (noflux)                                                      // row 0 of every frame's four planes
    for (int64_t i = (int64_t)blockIdx.x * LABEL_BLOCK + threadIdx.x; i < 4 * (int64_t)D.T; i += (int64_t)gridDim.x * LABEL_BLOCK)
      means[i * capacity] = i % 4 == 0 ? 1.0f : 0.0f;
  for (int64_t p = (int64_t)blockIdx.x * LABEL_BLOCK + threadIdx.x; p < D.NT; p += (int64_t)gridDim.x * LABEL_BLOCK) {
    if (lab[p] != (int)p) continue;
    const int64_t g = (int64_t)rank[p] + noflux;
    if (g >= capacity) continue;
    const int64_t f = frame_of(p, D), at = f * D.N;
    double d[4];
    for (int k = 0; k < 4; ++k) d[k] = (double)sums[4 * p + k];
    const double n2 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(d[0], d[0]), __dmul_rn(d[1], d[1])), __dmul_rn(d[2], d[2])), __dmul_rn(d[3], d[3]));
    const double len = __dsqrt_rn(n2);
    for (int k = 0; k < 4; ++k)
      means[(4 * f + k) * capacity + g] = n2 == 0.0 ? quats[4 * at + (int64_t)k * D.N + p - at] : (float)__ddiv_rn(d[k], len);
  }
}

// ---- the host routine: one map is a stack of one ------------------------------------------------------------------------------
struct LabelJob {
  const int32_t* ids;       // [T, ny, nx]                         (exactly one of ids, angles and quats)
  const float* angles;      // [T, K, ny, nx]
  const float* quats;       // [T, 4, ny, nx]
  const uint8_t* valid;     // [T, ny, nx] or NULL
  int32_t* image;           // [T, ny, nx]
  float* means;             // [T, K, capacity] (quats: [T, 4, capacity]); NULL with ids
  int64_t* status;          // [T, GGNN_LABEL_STATUS_WORDS]
  void* workspace;
  size_t workspace_bytes;
  int64_t T, nx, ny, capacity, min_pixels;
  float tol;                // angles: tol; quats: cos_half_tol
  int K;                    // channels of angles; 0 with ids and with quats
  int max_sweeps, boundary;
  bool cubic;
};

// what every entry point refuses in the same words: the sizes (T nx ny fits int32), the cleanup, the capacity, the boundary
static bool label_sizes_ok(int64_t T, int64_t nx, int64_t ny) {
  return T >= 1 && nx >= 3 && ny >= 3 && nx < (1 << 15) && ny < (1 << 15) && T <= INT32_MAX / (nx * ny);
}
static bool label_job_ok(const LabelJob& J) {
  if (!J.image || !J.status || !J.workspace || !label_sizes_ok(J.T, J.nx, J.ny)) return false;
  if (J.min_pixels < 1 || J.max_sweeps < 0 || J.max_sweeps > GGNN_LABEL_MAX_SWEEPS) return false;
  if (J.capacity < 1 || J.capacity >= INT32_MAX) return false;
  if (J.boundary != GGNN_BC_PERIODIC && J.boundary != GGNN_BC_NOFLUX) return false;
  if ((reinterpret_cast<uintptr_t>(J.status) & 7u) || (reinterpret_cast<uintptr_t>(J.workspace) & 7u)) return false;
  for (const void* p : {(const void*)J.image, (const void*)J.ids, (const void*)J.angles, (const void*)J.quats, (const void*)J.means})
    if (reinterpret_cast<uintptr_t>(p) & 3u) return false;
  return J.workspace_bytes >= label_carve(nullptr, nullptr, J.T, J.nx * J.ny, J.quats ? 4 : J.K);
}

// two memsets and 9 + 2 max_sweeps launches (quats: 12 + 2 max_sweeps), whatever T and whatever the maps hold
static int label_run(const LabelJob& J, hipStream_t st) {
  if (!label_job_ok(J)) return GGNN_EINVAL;
  const int64_t N = J.nx * J.ny, NT = J.T * N, chunks = (N + SCAN_CHUNK - 1) / SCAN_CHUNK;
  LabelWs W;
  label_carve(&W, (char*)J.workspace, J.T, N, J.quats ? 4 : J.K);
  const LabelDims D{(int)J.nx, (int)J.ny, (int)N, J.K, (int)J.T, (int)NT, (int)chunks, J.max_sweeps + 1, J.boundary == GGNN_BC_PERIODIC};
  const int noflux = D.periodic ? 0 : 1;
  if (hipMemsetAsync(J.status, 0, (size_t)J.T * GGNN_LABEL_STATUS_WORDS * sizeof(int64_t), st) != hipSuccess) return GGNN_ELAUNCH;
  if (hipMemsetAsync(W.words, 0, label_word_rows(J.T) * (size_t)D.wstride * sizeof(int32_t), st) != hipSuccess) return GGNN_ELAUNCH;
  // grids: from the device's CU count where a pass strides, from the work (T N <= INT32_MAX bounds every one) where it does not
  const int64_t wide = std::min<int64_t>((NT + LABEL_BLOCK - 1) / LABEL_BLOCK, 16 * (int64_t)num_cu());   // grid-stride passes
  const dim3 pass((unsigned)wide), block(LABEL_BLOCK);
  if (J.quats)
    hipLaunchKernelGGL(orient_links_kernel, pass, block, 0, st, J.quats, J.valid, W.links, D, J.tol, J.cubic);
  else if (J.angles)
    hipLaunchKernelGGL(label_links_kernel<true>, pass, block, 0, st, J.ids, J.angles, J.valid, W.links, D, J.tol);
  else
    hipLaunchKernelGGL(label_links_kernel<false>, pass, block, 0, st, J.ids, J.angles, J.valid, W.links, D, J.tol);
  const int tiles_x = (D.nx + LABEL_TX - 1) / LABEL_TX, tiles_y = (D.ny + LABEL_TY - 1) / LABEL_TY;
  const size_t lds = (size_t)LABEL_TILE * (8 + 8 * (size_t)J.K);
  hipLaunchKernelGGL(label_tile_kernel, dim3((unsigned)(J.T * tiles_x * tiles_y)), block, lds, st, J.angles, W.links, W.parent, W.size,
                     W.sums, J.status, D, tiles_x, tiles_x * tiles_y);
  const int64_t seams = J.T * ((int64_t)D.ny * tiles_x + (int64_t)D.nx * tiles_y);
  hipLaunchKernelGGL(label_seam_kernel, dim3((unsigned)std::min<int64_t>((seams + LABEL_BLOCK - 1) / LABEL_BLOCK, wide)), block, 0, st,
                     W.links, W.parent, J.status, D, tiles_x, tiles_y);
  hipLaunchKernelGGL(label_flatten_kernel, pass, block, 0, st, W.links, W.parent, W.size, W.sums, W.lab, J.status, D);
  hipLaunchKernelGGL(label_classify_kernel, pass, block, 0, st, W.links, W.size, W.lab, W.list, W.open, J.status, D, J.min_pixels);
  if (J.quats) {
    hipLaunchKernelGGL(orient_zero_kernel, pass, block, 0, st, W.lab, W.sums, D);    // (lab still marks the open pixels with -1)
    hipLaunchKernelGGL(orient_accumulate_kernel, pass, block, 0, st, J.quats, W.lab, W.sums, D, J.cubic ? GGNN_ORIENT_OPS : 1);
  }
  int32_t* pend = W.parent;                                       // (the parents are dead: every root is in lab)
  const dim3 few((unsigned)std::min<int64_t>(wide, 2 * (int64_t)num_cu()));   // (most sweeps return at once: a small grid strides the list)
  for (int s = 0; s < J.max_sweeps; ++s) {
    hipLaunchKernelGGL(label_decide_kernel, few, block, 0, st, W.lab, W.list, W.open, pend, W.words, D, s);
    hipLaunchKernelGGL(label_commit_kernel, few, block, 0, st, W.lab, W.list, W.open, pend, W.words, J.status, D, s);
  }
  const dim3 per_chunk((unsigned)(J.T * chunks));
  float* rank_means = J.quats ? nullptr : J.means;                // (the quaternion means are orient_means')
  hipLaunchKernelGGL(label_rank_sums_kernel, per_chunk, block, 0, st, W.lab, W.bsum, D);
  hipLaunchKernelGGL(label_rank_scan_kernel, dim3((unsigned)J.T), block, 0, st, W.bsum, chunks, J.status, rank_means, J.K, J.capacity, noflux);
  hipLaunchKernelGGL(label_rank_add_kernel, per_chunk, block, 0, st, W.lab, W.bsum, W.size, W.sums, W.rank, rank_means, D, J.capacity,
                     noflux);
  if (J.quats)
    hipLaunchKernelGGL(orient_means_kernel, pass, block, 0, st, J.quats, W.lab, W.rank, W.sums, J.means, D, J.capacity, noflux);
  hipLaunchKernelGGL(label_image_kernel, pass, block, 0, st, W.lab, W.rank, J.image, J.status, D, D.periodic ? 1 : 2);
  return launch_status();
}

template <class Args>
static int label_grains_run(const Args& A, int64_t T, ggnn_stream_t stream) {
  if ((A.ids != nullptr) == (A.angles != nullptr)) return GGNN_EINVAL;
  if (A.angles ? A.K < 1 || A.K > 4 || !A.mean_angles || !(A.tol >= 0.0f) : A.K != 0) return GGNN_EINVAL;
  return label_run(LabelJob{A.ids, A.angles, nullptr, A.valid, A.image, A.mean_angles, A.status, A.workspace, A.workspace_bytes, T, A.nx,
                            A.ny, A.grain_capacity, A.min_pixels, A.tol, A.K, A.max_sweeps, A.boundary, false},
                   (hipStream_t)stream);
}

template <class Args>
static int label_orient_run(const Args& A, int64_t T, ggnn_stream_t stream) {
  if (!A.quats || !A.mean_quats) return GGNN_EINVAL;
  if (!(A.cos_half_tol > GGNN_ORIENT_H && A.cos_half_tol <= 1.0f)) return GGNN_EINVAL;
  if (A.symmetry != GGNN_SYM_NONE && A.symmetry != GGNN_SYM_CUBIC) return GGNN_EINVAL;
  return label_run(LabelJob{nullptr, nullptr, A.quats, A.valid, A.image, A.mean_quats, A.status, A.workspace, A.workspace_bytes, T, A.nx,
                            A.ny, A.grain_capacity, A.min_pixels, A.cos_half_tol, 0, A.max_sweeps, A.boundary,
                            A.symmetry == GGNN_SYM_CUBIC},   // K = 0: the stages carry no angle sums
                   (hipStream_t)stream);
}

}  // namespace ggnn

extern "C" size_t ggnn_label_stack_workspace_bytes(int64_t T, int64_t nx, int64_t ny, int32_t K) {
  if (!ggnn::label_sizes_ok(T, nx, ny) || K < 0 || K > 4) return 0;
  return ggnn::label_carve(nullptr, nullptr, T, nx * ny, K);
}
extern "C" size_t ggnn_label_workspace_bytes(int64_t nx, int64_t ny, int32_t K) { return ggnn_label_stack_workspace_bytes(1, nx, ny, K); }

extern "C" int ggnn_label_grains_stack(const ggnn_label_stack_args* args, ggnn_stream_t stream) {
  return args ? ggnn::label_grains_run(*args, args->T, stream) : GGNN_EINVAL;
}
extern "C" int ggnn_label_grains(const ggnn_label_args* args, ggnn_stream_t stream) {
  return args ? ggnn::label_grains_run(*args, 1, stream) : GGNN_EINVAL;
}

extern "C" size_t ggnn_label_orient_stack_workspace_bytes(int64_t T, int64_t nx, int64_t ny) {
  return ggnn_label_stack_workspace_bytes(T, nx, ny, 4);
}
extern "C" size_t ggnn_label_orient_workspace_bytes(int64_t nx, int64_t ny) { return ggnn_label_stack_workspace_bytes(1, nx, ny, 4); }

extern "C" int ggnn_label_orientations_stack(const ggnn_label_orient_stack_args* args, ggnn_stream_t stream) {
  return args ? ggnn::label_orient_run(*args, args->T, stream) : GGNN_EINVAL;
}
extern "C" int ggnn_label_orientations(const ggnn_label_orient_args* args, ggnn_stream_t stream) {
  return args ? ggnn::label_orient_run(*args, 1, stream) : GGNN_EINVAL;
}
