// The junction graph of a grain-ID image, periodic or with no-flux walls: the inverse of raster.hip, and the way into a
// rollout for a structure that exists as an image (an EBSD map, a phase-field cross-section) and not as the reference's junction tracks
// (graph_trajectory.py:316-376 needs its solver's `node_region`).
//   ggnn_image_junctions = windows, representatives, numbering, positions, triples, grain->joint columns, status
//   ggnn_junction_links  = the joint->joint columns from the triples and the joint->grain table
//   ggnn_junction_links_trace_traj = the columns that rule leaves open because two grains meet twice, by following the boundary
// The rule is exact in integers up to the one fp32 expression of a position (include/ggnn.h; tests/vectorcheck.py restates
// it by brute force):
//   window (y, x) = pixels TL (y, x), TR (y, x + 1), BL (y + 1, x), BR (y + 1, x + 1), periodic; raster index y nx + x
//   keys          three distinct valid ids: that sorted triple; four: {TL, TR, BR} and {TL, BL, BR} (the TL-BR diagonal)
//   junction      a (window, key) with no window of a smaller raster index at an offset |dy|, |dx| <= R carrying the key
//   number        raster order of the window, ascending key within it
// A block is a segment of GGNN_JUNCTION_SEGMENT windows of one image row, so block order then thread order IS raster order:
// pass 1 counts the junctions of every block, one block scans the counts, pass 2 finds the same junctions again and writes
// them at scan[block] + the thread's rank in the block.  Nothing is kept between the passes but the counts: candidate
// windows are ~0.2 % of an image, their (2R + 1)^2 neighbourhood test reads the image through L2, and working it out
// twice costs less than a list of candidates would.  The numbering does not depend on the grid because nothing in it does:
// no atomics order anything (the three counters that use them are sums).
// GGNN_BC_NOFLUX is a compile-time mode of the same kernels (the periodic instantiation keeps its instruction stream): the
// windows run from -1, a pixel outside the image reads as the boundary grain's id 1 -- resolved in registers, no padded copy
// of the image is made --, offsets are clipped and not wrapped, and a junction of grain 0 gets its wall's coordinate exactly.
// STACK is a compile-time mode in the same way (ggnn_image_junctions_traj / ggnn_junction_links_traj: a stack of images into
// one union graph; the single-image instantiation keeps its instruction stream): the same rule per image and the same three
// passes, with the blocks laid out image-major -- block = image * (rows * segments) + row * segments + segment --, so block
// order is still the order of the numbering and the one scan block carries over; it also writes joint_off[image] = the scan at
// the image's first block.  A block belongs to one image: its base pointer, its grain range [grain_off[b], grain_off[b + 1])
// (clamped to the union's n_grain; read from the device, never from the host) and its status row are block-uniform, and the
// window tests run on that image alone, so a wrap, a clipped offset or an outside pixel never reaches a neighbouring image.
// The stack's count pass also counts the pixels per union grain (every pixel is the TL pixel of exactly one window): a lane
// adds the length of its run of equal ids in the wave, so a row inside a grain is one atomic and not 64.  A single image is
// the stack of one with the image's own ids: no grain_off and no joint_off exist for it, and every read or write of either
// stands in code that STACK = false compiles out.
// PINCH is a compile-time mode too (the _pinch_traj entry points; tests/pinchcheck.py restates it): GGNN_PINCH_NECK gives a
// window of three ids whose repeated id sits on a diagonal no key -- a grain's neck through a pixel corner is no junction --,
// in window_keys alone, which everything else reads; instantiated for stacks, and the default keeps its instruction stream.
// Every index is clamped as elsewhere: a pixel outside [1, n_grain] voids its windows, nothing is written at or beyond
// joint_capacity, and ggnn_junction_links bounds every row and column it reads by the tables' sizes.
#include <algorithm>

#include "common.h"
#include "segments.h"

namespace ggnn {

constexpr int VEC_BLOCK = GGNN_JUNCTION_SEGMENT;   // four waves, one window a thread
constexpr int VEC_WAVES = VEC_BLOCK / 64;
constexpr int VEC_SCAN_BLOCK = 1024;
constexpr int VEC_MAX_RADIUS = 7;
static_assert(VEC_BLOCK % 64 == 0, "whole waves");

__device__ __forceinline__ void sort3(int32_t& a, int32_t& b, int32_t& c) {
  const int32_t lo = min(a, min(b, c)), hi = max(a, max(b, c));
  b = a ^ b ^ c ^ lo ^ hi;   // (the middle one: the other two cancel)
  a = lo, c = hi;
}

__device__ __forceinline__ bool triple_less(const int32_t (&a)[3], const int32_t (&b)[3]) {
  return a[0] != b[0] ? a[0] < b[0] : a[1] != b[1] ? a[1] < b[1] : a[2] < b[2];
}

// Pixel (y, x) as the mode reads it.  Periodic: the image's own word (the caller has wrapped the indices).  No-flux: a pixel
// outside the image is the boundary grain's id 1; inside, id 1 reads as 0, which every test below takes for an invalid pixel
// (the boundary grain does not occur inside).  The load is from a clamped address and the choice a select: no lane branches
// on where it stands, and nothing is read outside the image.
template <int BC>
__device__ __forceinline__ int32_t pixel_at(const int32_t* __restrict__ image, int y, int x, int nx, int ny) {
  if (BC == GGNN_BC_PERIODIC) return image[(int64_t)y * nx + x];
  const bool inside = (unsigned)y < (unsigned)ny && (unsigned)x < (unsigned)nx;
  const int32_t v = image[(int64_t)min(max(y, 0), ny - 1) * nx + min(max(x, 0), nx - 1)];
  return inside ? (v == 1 ? 0 : v) : 1;
}

// The keys of window (y, x), 0-based grains, ascending: -> how many (0, 1 or 2 = a quadruple).  This is the one place that
// says what a window CARRIES.  PINCH = GGNN_PINCH_NECK: a window of three distinct valid ids whose repeated id sits on a
// diagonal ([a b; c a] or [b a; a c]: grain a runs through the corner as a neck one pixel wide) carries nothing, and `pinch`
// says so, false for every other window; GGNN_PINCH_JUNCTION never writes it, and its instruction stream is the one it was.
template <int BC, int PINCH>
__device__ __forceinline__ int window_keys(const int32_t* __restrict__ image, int y, int x, int nx, int ny, int32_t n_grain,
                                           int32_t (&k)[2][3], bool& tl_invalid, bool& pinch) {
  const int x1 = BC == GGNN_BC_PERIODIC && x + 1 == nx ? 0 : x + 1, y1 = BC == GGNN_BC_PERIODIC && y + 1 == ny ? 0 : y + 1;
  const int32_t tl = pixel_at<BC>(image, y, x, nx, ny), tr = pixel_at<BC>(image, y, x1, nx, ny);
  const int32_t bl = pixel_at<BC>(image, y1, x, nx, ny), br = pixel_at<BC>(image, y1, x1, nx, ny);
  tl_invalid = tl < 1 || tl > n_grain;
  if (PINCH == GGNN_PINCH_NECK) pinch = false;
  if (tl == tr && tl == bl && tl == br) return 0;
  if (tl_invalid || tr < 1 || tr > n_grain || bl < 1 || bl > n_grain || br < 1 || br > n_grain) return 0;
  const bool e01 = tl == tr, e02 = tl == bl, e03 = tl == br, e12 = tr == bl, e13 = tr == br, e23 = bl == br;
  const int equal = e01 + e02 + e03 + e12 + e13 + e23;   // 0: four distinct ids, 1: three, more: fewer
  if (equal > 1) return 0;
  if (equal == 1) {   // the three distinct ones: all but the second pixel of the equal pair
    if (PINCH == GGNN_PINCH_NECK && (e03 || e12)) {
      pinch = true;
      return 0;
    }
    k[0][0] = tl - 1;
    k[0][1] = (e01 ? bl : tr) - 1;
    k[0][2] = (e01 || e02 || e12 ? br : bl) - 1;
    sort3(k[0][0], k[0][1], k[0][2]);
    return 1;
  }
  k[0][0] = tl - 1, k[0][1] = tr - 1, k[0][2] = br - 1;
  k[1][0] = tl - 1, k[1][1] = bl - 1, k[1][2] = br - 1;
  sort3(k[0][0], k[0][1], k[0][2]);
  sort3(k[1][0], k[1][1], k[1][2]);
  if (triple_less(k[1], k[0]))
    for (int i = 0; i < 3; ++i) {
      const int32_t t = k[0][i];
      k[0][i] = k[1][i], k[1][i] = t;
    }
  return 2;
}

template <int BC, int PINCH>
__device__ __forceinline__ bool window_carries(const int32_t* __restrict__ image, int y, int x, int nx, int ny, int32_t n_grain,
                                               const int32_t (&key)[3]) {
  int32_t k[2][3];
  bool unused, no_key = false;
  const int n = window_keys<BC, PINCH>(image, y, x, nx, ny, n_grain, k, unused, no_key);
  for (int i = 0; i < n; ++i)
    if (k[i][0] == key[0] && k[i][1] == key[1] && k[i][2] == key[2]) return true;
  return false;
}

// Is window (y, x) the representative of `key`; m, sx, sy = the carriers at offsets within R (itself included) and the sums
// of their offsets.  Periodic: the offsets wrap.  No-flux: the window range [-1, ny - 1] x [-1, nx - 1] clips them.
template <int BC, int PINCH>
__device__ __forceinline__ bool window_represents(const int32_t* __restrict__ image, int y, int x, int nx, int ny, int32_t n_grain,
                                                  int R, const int32_t (&key)[3], int& m, int& sx, int& sy) {
  bool rep = true;
  m = 1, sx = 0, sy = 0;
  for (int dy = -R; dy <= R; ++dy) {
    int yy = y + dy;
    if (BC == GGNN_BC_PERIODIC)
      yy += yy < 0 ? ny : yy >= ny ? -ny : 0;   // (ny > 2 R: one step)
    else if (yy < -1 || yy >= ny)
      continue;
    for (int dx = -R; dx <= R; ++dx) {
      if (dy == 0 && dx == 0) continue;
      int xx = x + dx;
      if (BC == GGNN_BC_PERIODIC)
        xx += xx < 0 ? nx : xx >= nx ? -nx : 0;
      else if (xx < -1 || xx >= nx)
        continue;
      if (!window_carries<BC, PINCH>(image, yy, xx, nx, ny, n_grain, key)) continue;
      if (yy < y || (yy == y && xx < x)) rep = false;   // a smaller raster index
      ++m, sx += dx, sy += dy;
    }
  }
  return rep;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
  return v;
}

// What the kernels of both junction entry points take, filled from the public structs.  A single image: n_image 1, no
// grain_off, no rep, pixel_counts = the caller's histogram by id (read); a stack: pixel_counts by union grain (written).
struct junction_kargs {
  const int32_t* images;         // [n_image, ny, nx]
  const int64_t* grain_off;      // [n_image + 1], STACK alone
  uint64_t* pixel_counts;
  float* xy;
  int32_t* triples;
  int64_t* edge_gj;
  int64_t* status;               // the caller's: n_image rows, and for STACK joint_off [n_image + 1] behind them
  int32_t* workspace;            // a word a block
  int32_t* rep;                  // ggnn_image_junction_windows_traj's, or null
  int64_t nx, ny, n_image, n_grain, joint_capacity;
  float offset, pitch;
  int32_t merge_radius;
  int32_t segments, rows;        // the blocks of a row of windows, the rows of windows of an image
  int64_t* pinch_windows;        // [n_image], PINCH = GGNN_PINCH_NECK alone: the pinch windows of every image
};

// The grains of image b: -> the first one, n = how many (0 when the offsets do not rise).
__device__ __forceinline__ int64_t image_grains(const int64_t* __restrict__ grain_off, int64_t b, int64_t n_total, int32_t& n) {
  const int64_t lo = min(max(grain_off[b], (int64_t)0), n_total), hi = min(max(grain_off[b + 1], lo), n_total);
  n = (int32_t)(hi - lo);
  return lo;
}

// EMIT = false: block_count[b] = the junctions of block b, the three window counters of the status and, for a stack, the
//               pixel counts.
// EMIT = true : block_count holds the exclusive scan; the junctions are written.
// BC = GGNN_BC_NOFLUX: the grid is ny + 1 rows of segments of the nx + 1 windows of a row, and window (y, x) begins at -1.
// STACK = false: the image is the one image, its grains are 0 .. n_grain - 1 and its status row is the one row.
// PINCH = GGNN_PINCH_NECK (stacks alone): the count pass also sums the pinch windows of every image, as it does the quadruples.
template <bool EMIT, int BC, bool STACK, int PINCH = GGNN_PINCH_JUNCTION>
__global__ __launch_bounds__(VEC_BLOCK) void image_junctions_kernel(const junction_kargs A) {
  __shared__ int wave_total[VEC_WAVES];
  constexpr int FIRST = BC == GGNN_BC_PERIODIC ? 0 : -1;
  const int nx = (int)A.nx, ny = (int)A.ny, R = A.merge_radius, segments = A.segments;
  int b = 0;
  unsigned in_image = blockIdx.x;
  int32_t n_grain = (int32_t)A.n_grain;
  int64_t g0 = 0;
  const int32_t* __restrict__ image = A.images;
  if (STACK) {   // (block-uniform)
    const int per_image = A.rows * segments;
    b = blockIdx.x / per_image, in_image = blockIdx.x - b * per_image;
    if (b >= A.n_image) return;
    g0 = image_grains(A.grain_off, b, A.n_grain, n_grain);
    image += (int64_t)b * ny * nx;
  }
  const int row = in_image / segments;
  const int y = row + FIRST, x = (in_image - row * segments) * VEC_BLOCK + threadIdx.x + FIRST;
  int32_t k[2][3];
  int n_keys = 0, m[2] = {0, 0}, sx[2] = {0, 0}, sy[2] = {0, 0};
  bool rep[2] = {false, false}, tl_invalid = false, pinch = false;   // (pinch: window_keys<.., GGNN_PINCH_JUNCTION> leaves it)
  if (x < nx) {
    n_keys = window_keys<BC, PINCH>(image, y, x, nx, ny, n_grain, k, tl_invalid, pinch);
    for (int i = 0; i < n_keys; ++i)
      rep[i] = window_represents<BC, PINCH>(image, y, x, nx, ny, n_grain, R, k[i], m[i], sx[i], sy[i]);
  }
  const int mine = (rep[0] ? 1 : 0) + (rep[1] ? 1 : 0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t one = __ballot(mine >= 1), two = __ballot(mine == 2);
  if (lane == 0) wave_total[wave] = __popcll(one) + __popcll(two);
  __syncthreads();
  if (!EMIT) {
    if (threadIdx.x == 0) {
      int total = 0;
      for (int w = 0; w < VEC_WAVES; ++w) total += wave_total[w];
      A.workspace[blockIdx.x] = total;
    }
    unsigned long long* status = (unsigned long long*)A.status + (int64_t)b * GGNN_JUNCTION_STATUS_WORDS;
    const unsigned long long quads = wave_sum(n_keys == 2 ? 1 : 0), merged = wave_sum((unsigned long long)(n_keys - mine)),
                             invalid = wave_sum(tl_invalid ? 1 : 0);
    if (lane == 0) {
      if (quads) atomicAdd(status + 1, quads);
      if (merged) atomicAdd(status + 2, merged);
      if (invalid) atomicAdd(status + 3, invalid);
    }
    if (PINCH == GGNN_PINCH_NECK) {
      const unsigned long long pinches = wave_sum(pinch ? 1 : 0);
      if (lane == 0 && pinches) atomicAdd((unsigned long long*)A.pinch_windows + b, pinches);
    }
    if (STACK) {
      // the pixel counts: the image's own word of the TL pixel (id 1 of a no-flux image included: the counts are a histogram)
      int32_t id = 0;
      if (x < nx && x >= 0 && y >= 0) {
        id = image[(int64_t)y * nx + x];
        id = id >= 1 && id <= n_grain ? id : 0;
      }
      const int32_t before = __shfl_up(id, 1);
      const bool head = lane == 0 || id != before;
      const uint64_t heads = __ballot(head);
      if (head && id) {
        const uint64_t above = lane == 63 ? 0 : heads >> (lane + 1);
        const int run = above ? __ffsll((unsigned long long)above) : 64 - lane;
        atomicAdd((unsigned long long*)A.pixel_counts + g0 + id - 1, (unsigned long long)run);
      }
    }
    return;
  }
  if (!mine) return;
  const uint64_t below = lane ? ~0ull >> (64 - lane) : 0;
  int64_t j = (int64_t)A.workspace[blockIdx.x] + __popcll(one & below) + __popcll(two & below);
  for (int w = 0; w < wave; ++w) j += wave_total[w];
  const int64_t ld = 3 * A.joint_capacity;
  for (int i = 0; i < n_keys; ++i) {
    if (!rep[i]) continue;
    if (j >= 0 && j < A.joint_capacity) {
      // x = ((float)xr + off + (float)Sx / (float)m) * pitch: the quotient, the sum of the first two, the sum, the product
      const float qx = __fdiv_rn((float)sx[i], (float)m[i]), qy = __fdiv_rn((float)sy[i], (float)m[i]);
      float px = __fmul_rn(__fadd_rn(__fadd_rn((float)x, A.offset), qx), A.pitch);
      float py = __fmul_rn(__fadd_rn(__fadd_rn((float)y, A.offset), qy), A.pitch);
      if (BC == GGNN_BC_NOFLUX && k[i][0] == 0) {   // a wall junction: the wall its window straddles sets the coordinate
        const float two_off = __fmul_rn(2.0f, A.offset);
        const float max_y = __fdiv_rn(__fadd_rn((float)(ny - 2), two_off), __fadd_rn((float)(nx - 2), two_off));
        px = x == -1 ? 0.0f : x == nx - 1 ? 1.0f : fminf(fmaxf(px, 0.0f), 1.0f);
        py = y == -1 ? 0.0f : y == ny - 1 ? max_y : fminf(fmaxf(py, 0.0f), max_y);
      }
      A.xy[2 * j] = px;
      A.xy[2 * j + 1] = py;
      for (int c = 0; c < 3; ++c) {
        const int64_t g = g0 + k[i][c];   // (below the union's n_grain < 2^31)
        A.triples[3 * j + c] = (int32_t)g;
        A.edge_gj[3 * j + c] = g;
        A.edge_gj[ld + 3 * j + c] = j;
      }
      // (ggnn_image_junction_windows_traj: the representative's raster index within its image, below 2^30)
      if (STACK && A.rep) A.rep[j] = BC == GGNN_BC_PERIODIC ? y * nx + x : (y + 1) * (nx + 1) + (x + 1);
    }
    ++j;
  }
}

// One block: the exclusive scan of the block counts in place; per image n_joint, overflow and the grains that have pixels
// (local grains from first_local: 0, or 1 for a no-flux image, whose local grain 0 is the boundary grain) and, for a stack,
// joint_off behind the status rows.  A stack's present grains are summed in LDS for the first VEC_SCAN_BLOCK images, in
// memory beyond; a single image's are the ids first_local + 1 .. n_grain of its histogram, summed by wave.
template <bool STACK>
__global__ __launch_bounds__(VEC_SCAN_BLOCK) void junction_scan_kernel(const junction_kargs A, int64_t first_local) {
  __shared__ long long part[VEC_SCAN_BLOCK];
  __shared__ unsigned int present[STACK ? VEC_SCAN_BLOCK : 1];
  int32_t* __restrict__ count = A.workspace;
  int64_t* __restrict__ status = A.status;
  const int64_t n_image = STACK ? A.n_image : 1, per_image = (int64_t)A.rows * A.segments, n_blocks = n_image * per_image;
  const int64_t n_grain = A.n_grain, joint_capacity = A.joint_capacity;
  const int t = threadIdx.x;
  const int64_t per = (n_blocks + VEC_SCAN_BLOCK - 1) / VEC_SCAN_BLOCK;
  const int64_t begin = min((int64_t)t * per, n_blocks), end = min(begin + per, n_blocks);
  long long sum = 0;
  for (int64_t i = begin; i < end; ++i) sum += count[i];
  part[t] = sum;
  if (STACK || t == 0) present[STACK ? t : 0] = 0;
  __syncthreads();
  for (int s = 1; s < VEC_SCAN_BLOCK; s <<= 1) {   // inclusive scan of the threads' sums
    const long long add = t >= s ? part[t - s] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  long long at = part[t] - sum;
  for (int64_t i = begin; i < end; ++i) {
    const int32_t c = count[i];
    count[i] = (int32_t)at;   // (at most 512 junctions a block, at most 2^22 blocks)
    at += c;
  }
  if (STACK) {
    const uint64_t* __restrict__ pixel_counts = A.pixel_counts;
    for (int64_t g = t; g < n_grain; g += VEC_SCAN_BLOCK) {
      if (pixel_counts[g] == 0) continue;
      const int64_t b = seg_of(A.grain_off, (int)n_image, g);
      int32_t n;
      const int64_t g0 = image_grains(A.grain_off, b, n_grain, n);
      if (g < g0 + first_local || g >= g0 + n) continue;
      if (b < VEC_SCAN_BLOCK)
        atomicAdd(&present[b], 1u);
      else
        atomicAdd((unsigned long long*)status + b * GGNN_JUNCTION_STATUS_WORDS + 5, 1ull);
    }
  } else {
    const uint64_t* __restrict__ by_id = A.pixel_counts + 1;
    unsigned long long have = 0;
    for (int64_t g = first_local + t; g < n_grain; g += VEC_SCAN_BLOCK) have += by_id[g] != 0 ? 1 : 0;
    have = wave_sum(have);   // (below n_grain < 2^31)
    if ((t & 63) == 0 && have) atomicAdd(&present[0], (unsigned int)have);
  }
  __syncthreads();   // (the scan in `count` and the LDS sums, for every thread of the block)
  const long long total = part[VEC_SCAN_BLOCK - 1];
  int64_t* joint_off = status + n_image * GGNN_JUNCTION_STATUS_WORDS;   // (STACK alone: a single image's status ends here)
  for (int64_t b = t; b < n_image; b += VEC_SCAN_BLOCK) {
    const long long lo = count[b * per_image], hi = b + 1 < n_image ? (long long)count[(b + 1) * per_image] : total;
    int64_t* s = status + b * GGNN_JUNCTION_STATUS_WORDS;
    if (STACK) joint_off[b] = lo;
    s[0] = hi - lo;
    if (b < VEC_SCAN_BLOCK) s[5] = present[b];
    s[6] = hi > joint_capacity ? 1 : 0;
  }
  if (STACK && t == 0) joint_off[n_image] = total;
}

__global__ __launch_bounds__(256) void zero_open_pairs_kernel(int64_t* __restrict__ status, int64_t n_image) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < n_image) status[b * GGNN_JUNCTION_STATUS_WORDS + 4] = 0;
}

// One thread a (junction, pair) slot: the one other junction of grain a's row whose triple holds grain b.  On a union the
// triples and rows hold union grains, a pair's partner lies in its grain's row and so in its image.  An open slot is counted
// in word 4 of its image's status row: the one row, or the row of the image that joint_off puts the junction in.  (The
// arguments are the union's for both: ggnn_junction_links fills them with n_image 1.)
template <bool STACK>
__global__ __launch_bounds__(256) void junction_links_kernel(const ggnn_link_traj_args A) {
  const int64_t* joint_off = A.status + A.n_image * GGNN_JUNCTION_STATUS_WORDS;   // (STACK alone)
  const int64_t n = min(max(STACK ? joint_off[A.n_image] : A.status[0], (int64_t)0), A.joint_capacity);
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= 3 * n) return;
  const int64_t j = s / 3;
  const int k = (int)(s - 3 * j);
  const int32_t a = A.triples[3 * j + (k == 2 ? 1 : 0)], b = A.triples[3 * j + (k == 0 ? 1 : 2)];
  int found = 0;
  int64_t partner = -1;
  if (a >= 0 && a < A.n_grain) {
    const int64_t p0 = min((int64_t)max(A.rowptr[a], 0), A.E_cap);
    const int64_t p1 = min(max((int64_t)A.rowptr[a + 1], p0), A.E_cap);
    for (int64_t p = p0; p < p1; ++p) {
      const int64_t o = A.col[p];
      if (o < 0 || o >= n || o == j) continue;
      if (A.triples[3 * o] == b || A.triples[3 * o + 1] == b || A.triples[3 * o + 2] == b) ++found, partner = o;
    }
  }
  A.edge_jj[s] = j;
  A.edge_jj[3 * A.joint_capacity + s] = found == 1 ? partner : -1;
  if (found != 1)   // (rare: none in a valid structure)
    atomicAdd((unsigned long long*)A.status + (STACK ? seg_of(joint_off, (int)A.n_image, j) : 0) * GGNN_JUNCTION_STATUS_WORDS + 4,
              1ull);
}

// ---- Linking by tracing boundaries (ggnn_junction_links_trace_traj; tests/tracecheck.py restates the rule) ------------------
// The columns junction_links_kernel<true> left open -- a pair of grains held by more than one other junction: a lens on a
// boundary, a band from wall to wall -- are linked by following the a | b boundary through the image, pixel edge by pixel
// edge, from the junction to the one at the other end.  A thread takes a column and returns at once unless it is open; the
// open ones are a handful an image and each is a chain of dependent reads that L2 serves, so there is no compaction and no
// tile: the few lanes that walk do so alone, and a wave without an open column is done after one load.  Every loop is
// bounded: the neighbourhoods by (2R + 1)^2, a row of the table by E_cap, the walk by max_trace.  A thread writes its own
// column only and reads no other's, so the reverse column is found by its own thread, which walks the same chain backwards.
constexpr int TRACE_TRACED = 0, TRACE_FAILED = 1, TRACE_OVERFLOW = 2;
// The three large helpers stay OUT OF LINE.  Inlined into one body (some 7000 instructions, exits worked out at two places
// inside the walk) the periodic instantiation spilled over a hundred scalar registers into vector lanes across its nested
// divergent loops and, at -O3 on gfx950, failed every walk along a horizontal stretch of boundary, while the same source links
// them on the host (plain and under the address, undefined-behaviour and memory sanitizers), at -O1, and out of line.  As
// calls the kernel is a fifth of the size, and the path is a rare one (tests/test_trace_links.py walks both directions).
#define TRACE_FN __device__ __attribute__((noinline))

struct trace_image {             // the image of a column, as its thread sees it
  const int32_t* image;          // [ny, nx]
  const int32_t* triples;        // the union's
  const int32_t* rep;
  const int32_t* rowptr;
  const int32_t* col;
  int64_t g0, n_total;           // the image's first union grain; the union's grains
  int64_t j_lo, j_hi;            // the image's junctions that were kept
  int64_t E_cap;
  int32_t n_grain;               // the image's
  int nx, ny, R;
};

// The window of raster index r -> is it one.
template <int BC>
__device__ bool trace_window(const trace_image& I, int32_t r, int& y, int& x) {
  const int w = BC == GGNN_BC_PERIODIC ? I.nx : I.nx + 1, h = BC == GGNN_BC_PERIODIC ? I.ny : I.ny + 1;
  if (r < 0 || (int64_t)r >= (int64_t)w * h) return false;
  y = r / w, x = r - y * w;
  if (BC == GGNN_BC_NOFLUX) --y, --x;
  return true;
}

template <int BC>
__device__ __forceinline__ bool trace_in_range(const trace_image& I, int y, int x) {
  return BC == GGNN_BC_PERIODIC ? (unsigned)y < (unsigned)I.ny && (unsigned)x < (unsigned)I.nx
                                : y >= -1 && y < I.ny && x >= -1 && x < I.nx;
}

// Does (yb, xb) lie at an offset within R of (ya, xa): the minimum image, or the plain difference between walls.
template <int BC>
__device__ __forceinline__ bool trace_near(const trace_image& I, int ya, int xa, int yb, int xb) {
  int dy = yb - ya, dx = xb - xa;
  if (BC == GGNN_BC_PERIODIC) {
    dy += dy < 0 ? I.ny : 0, dx += dx < 0 ? I.nx : 0;
    return (dy <= I.R || dy >= I.ny - I.R) && (dx <= I.R || dx >= I.nx - I.R);
  }
  return dy >= -I.R && dy <= I.R && dx >= -I.R && dx <= I.R;
}

// The vertex across crack d (UP, DOWN, LEFT, RIGHT) of (y, x): wrapped on the torus, as it is between walls (the caller
// tests the range before it reads there).
template <int BC>
__device__ __forceinline__ void trace_step(const trace_image& I, int y, int x, int d, int& y2, int& x2) {
  y2 = y + (d == 0 ? -1 : d == 1 ? 1 : 0), x2 = x + (d == 2 ? -1 : d == 3 ? 1 : 0);
  if (BC == GGNN_BC_PERIODIC) {
    y2 += y2 < 0 ? I.ny : y2 >= I.ny ? -I.ny : 0;
    x2 += x2 < 0 ? I.nx : x2 >= I.nx ? -I.nx : 0;
  }
}

// The four pixels TL, TR, BL, BR of an in-range window, and its a | b cracks as a mask of UP, DOWN, LEFT, RIGHT.
template <int BC>
__device__ int trace_cracks(const trace_image& I, int y, int x, int32_t ia, int32_t ib, int32_t (&px)[4]) {
  const int x1 = BC == GGNN_BC_PERIODIC && x + 1 == I.nx ? 0 : x + 1, y1 = BC == GGNN_BC_PERIODIC && y + 1 == I.ny ? 0 : y + 1;
  px[0] = pixel_at<BC>(I.image, y, x, I.nx, I.ny), px[1] = pixel_at<BC>(I.image, y, x1, I.nx, I.ny);
  px[2] = pixel_at<BC>(I.image, y1, x, I.nx, I.ny), px[3] = pixel_at<BC>(I.image, y1, x1, I.nx, I.ny);
  const auto ab = [&](int p, int q) { return (px[p] == ia && px[q] == ib) || (px[p] == ib && px[q] == ia); };
  return (ab(0, 1) ? 1 : 0) | (ab(2, 3) ? 2 : 0) | (ab(0, 2) ? 4 : 0) | (ab(1, 3) ? 8 : 0);
}

// The junction that owns the carrier (y, x) of the local key: the smallest kept one of the image with that triple whose
// representative lies within R, found in the joint->grain row of the key's last grain (never a no-flux boundary grain, whose
// row holds every wall junction); -1: nobody.
template <int BC>
TRACE_FN int64_t trace_owner(const trace_image& I, int y, int x, const int32_t (&key)[3]) {
  const int64_t g = I.g0 + key[2];
  if (g < 0 || g >= I.n_total) return -1;
  const int64_t p0 = min((int64_t)max(I.rowptr[g], 0), I.E_cap);
  const int64_t p1 = min(max((int64_t)I.rowptr[g + 1], p0), I.E_cap);
  int64_t best = -1;
  for (int64_t p = p0; p < p1; ++p) {
    const int64_t o = I.col[p];
    if (o < I.j_lo || o >= I.j_hi || (best >= 0 && o > best)) continue;
    if (I.triples[3 * o] != I.g0 + key[0] || I.triples[3 * o + 1] != I.g0 + key[1] || I.triples[3 * o + 2] != g) continue;
    int ry, rx;
    if (!trace_window<BC>(I, I.rep[o], ry, rx) || !trace_near<BC>(I, ry, rx, y, x)) continue;
    best = o;
  }
  return best;
}

template <int BC, int PINCH>
__device__ bool trace_owned(const trace_image& I, int64_t j, const int32_t (&key)[3], int y, int x) {
  return trace_in_range<BC>(I, y, x) && window_carries<BC, PINCH>(I.image, y, x, I.nx, I.ny, I.n_grain, key) &&
         trace_owner<BC>(I, y, x, key) == j;
}

// The exits of junction j (local key) for the ids ia, ib -> how many, the last one as the vertex reached and the crack taken;
// n_diag, (qy, qx): the quadruple windows owned by j whose TL and BR are the two ids, and the last of them.
template <int BC, int PINCH>
TRACE_FN int trace_exits(const trace_image& I, int64_t j, const int32_t (&key)[3], int32_t ia, int32_t ib, int& ey, int& ex,
                           int& ed, int& n_diag, int& qy, int& qx) {
  int n = 0, ry, rx;
  n_diag = 0;
  if (!trace_window<BC>(I, I.rep[j], ry, rx)) return 0;
  for (int dy = -I.R; dy <= I.R; ++dy)
    for (int dx = -I.R; dx <= I.R; ++dx) {
      int y = ry + dy, x = rx + dx;
      if (BC == GGNN_BC_PERIODIC) {
        y += y < 0 ? I.ny : y >= I.ny ? -I.ny : 0;
        x += x < 0 ? I.nx : x >= I.nx ? -I.nx : 0;
      }
      if (!trace_owned<BC, PINCH>(I, j, key, y, x)) continue;
      int32_t px[4];
      const int cracks = trace_cracks<BC>(I, y, x, ia, ib, px);
      const bool quad = px[0] != px[1] && px[0] != px[2] && px[0] != px[3] && px[1] != px[2] && px[1] != px[3] && px[2] != px[3];
      if (quad && ((px[0] == ia && px[3] == ib) || (px[0] == ib && px[3] == ia))) ++n_diag, qy = y, qx = x;
      for (int d = 0; d < 4; ++d) {
        if (!(cracks >> d & 1)) continue;
        int y2, x2;
        trace_step<BC>(I, y, x, d, y2, x2);
        if (!trace_owned<BC, PINCH>(I, j, key, y2, x2)) ++n, ey = y2, ex = x2, ed = d;
      }
    }
  return n;
}

// The partner of junction j (local key) for its local grains a, b -> TRACE_*; o: the partner when traced.
template <int BC, int PINCH>
TRACE_FN int trace_partner(const trace_image& I, int64_t j, const int32_t (&key)[3], int32_t a, int32_t b, int64_t max_trace,
                             int64_t& o) {
  const int32_t ia = a + 1, ib = b + 1;
  int y = 0, x = 0, d = 0, n_diag, qy = 0, qx = 0;
  const int n_exit = trace_exits<BC, PINCH>(I, j, key, ia, ib, y, x, d, n_diag, qy, qx);
  int32_t k[2][3];
  bool unused, no_key = false;
  if (n_diag) {   // the diagonal of a quadruple window: its two junctions, when each has this one diagonal
    if (n_diag != 1) return TRACE_FAILED;
    if (window_keys<BC, PINCH>(I.image, qy, qx, I.nx, I.ny, I.n_grain, k, unused, no_key) != 2) return TRACE_FAILED;
    const int other = k[0][0] == key[0] && k[0][1] == key[1] && k[0][2] == key[2] ? 1 : 0;
    o = trace_owner<BC>(I, qy, qx, k[other]);
    if (o < 0 || o == j) return TRACE_FAILED;
    int ty, tx, td, their_diag, ry = 0, rx = 0;
    trace_exits<BC, PINCH>(I, o, k[other], ia, ib, ty, tx, td, their_diag, ry, rx);
    return their_diag == 1 && ry == qy && rx == qx ? TRACE_TRACED : TRACE_FAILED;
  }
  if (n_exit != 1) return TRACE_FAILED;
  int arrived = d ^ 1;   // (UP <-> DOWN, LEFT <-> RIGHT)
  for (int64_t steps = 1;; ++steps) {
    if (steps > max_trace) return TRACE_OVERFLOW;
    if (!trace_in_range<BC>(I, y, x)) return TRACE_FAILED;
    const int n_keys = window_keys<BC, PINCH>(I.image, y, x, I.nx, I.ny, I.n_grain, k, unused, no_key);
    for (int i = 0; i < n_keys; ++i) {
      const bool has_a = k[i][0] == a || k[i][1] == a || k[i][2] == a, has_b = k[i][0] == b || k[i][1] == b || k[i][2] == b;
      if (!(has_a && has_b)) continue;
      o = trace_owner<BC>(I, y, x, k[i]);   // the junction at the other end
      if (o < 0 || o == j) return TRACE_FAILED;
      int ty, tx, td, their_diag, ry, rx;
      const int theirs = trace_exits<BC, PINCH>(I, o, k[i], ia, ib, ty, tx, td, their_diag, ry, rx);
      return their_diag == 0 && theirs == 1 ? TRACE_TRACED : TRACE_FAILED;
    }
    int32_t px[4];
    const int cracks = trace_cracks<BC>(I, y, x, ia, ib, px);
    if (__popc(cracks) != 2 || !(cracks >> arrived & 1)) return TRACE_FAILED;   // (one: a dead end; four: [a b; b a])
    d = __ffs(cracks & ~(1 << arrived)) - 1;
    int y2, x2;
    trace_step<BC>(I, y, x, d, y2, x2);
    y = y2, x = x2, arrived = d ^ 1;
  }
}

template <int BC, int PINCH = GGNN_PINCH_JUNCTION>
__global__ __launch_bounds__(256) void junction_trace_kernel(const ggnn_link_trace_args A) {
  const int64_t* joint_off = A.status + A.n_image * GGNN_JUNCTION_STATUS_WORDS;
  const int64_t n = min(max(joint_off[A.n_image], (int64_t)0), A.joint_capacity);
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= 3 * n) return;
  int64_t* slot = A.edge_jj + 3 * A.joint_capacity + s;
  if (*slot != -1) return;   // (every column of a structure without open pairs)
  const int64_t j = s / 3;
  const int c = (int)(s - 3 * j);
  const int64_t b = seg_of(joint_off, (int)A.n_image, j);
  trace_image I;
  I.g0 = image_grains(A.grain_off, b, A.n_grain, I.n_grain);
  I.image = A.images + b * A.ny * A.nx;
  I.triples = A.triples, I.rep = A.rep, I.rowptr = A.rowptr, I.col = A.col;
  I.n_total = A.n_grain, I.E_cap = A.E_cap;
  I.j_lo = min(max(joint_off[b], (int64_t)0), n), I.j_hi = min(max(joint_off[b + 1], I.j_lo), n);
  I.nx = (int)A.nx, I.ny = (int)A.ny, I.R = A.merge_radius;
  int32_t key[3];
  bool inside = true;
  for (int i = 0; i < 3; ++i) {
    const int64_t g = (int64_t)A.triples[3 * j + i] - I.g0;
    inside = inside && g >= 0 && g < I.n_grain;
    key[i] = (int32_t)g;
  }
  int64_t o = -1;
  const int what = inside ? trace_partner<BC, PINCH>(I, j, key, key[c == 2 ? 1 : 0], key[c == 0 ? 1 : 2], A.max_trace, o) : TRACE_FAILED;
  atomicAdd((unsigned long long*)A.counters + GGNN_TRACE_COUNTERS * b + what, 1ull);
  if (what != TRACE_TRACED) return;
  *slot = o;
  atomicAdd((unsigned long long*)A.status + b * GGNN_JUNCTION_STATUS_WORDS + 4, ~0ull);   // one open pair fewer
}

}  // namespace ggnn

// The checks the junction entry points share, on the kernel arguments they filled: -> the blocks of the grid, with
// K.segments and K.rows set, or 0: invalid.  (A single image, n_image 1, has at most 2^15 2^7 = GGNN_JUNCTION_MAX_BLOCKS.)
static int64_t junction_blocks(ggnn::junction_kargs& K, size_t workspace_bytes, int32_t boundary) {
  using namespace ggnn;
  if (!K.images || !K.pixel_counts || !K.xy || !K.triples || !K.edge_gj || !K.status || !K.workspace) return 0;
  if (K.merge_radius < 0 || K.merge_radius > VEC_MAX_RADIUS) return 0;
  if (K.nx <= 2 * K.merge_radius || K.ny <= 2 * K.merge_radius || K.nx >= (1 << 15) || K.ny >= (1 << 15)) return 0;
  if (K.n_image < 1 || K.n_image > GGNN_JUNCTION_MAX_BLOCKS) return 0;
  if (K.n_grain < 1 || K.n_grain >= INT32_MAX - 1) return 0;
  if (K.joint_capacity < 1 || K.joint_capacity > INT32_MAX / 3) return 0;
  if (!(K.pitch > 0.0f) || !(K.offset >= 0.0f) || K.pitch > 1.0f || K.offset > 1.0f) return 0;
  if ((reinterpret_cast<uintptr_t>(K.status) | reinterpret_cast<uintptr_t>(K.edge_gj) |
       reinterpret_cast<uintptr_t>(K.pixel_counts)) & 7u)
    return 0;
  if (boundary != GGNN_BC_PERIODIC && boundary != GGNN_BC_NOFLUX) return 0;
  const bool periodic = boundary == GGNN_BC_PERIODIC;
  const int64_t wx = periodic ? K.nx : K.nx + 1, wy = periodic ? K.ny : K.ny + 1;   // the windows of a row, the rows
  K.segments = (int32_t)((wx + VEC_BLOCK - 1) / VEC_BLOCK), K.rows = (int32_t)wy;
  const int64_t n_blocks = K.n_image * wy * K.segments;                             // (< 2^22 2^22: no overflow)
  if (n_blocks > GGNN_JUNCTION_MAX_BLOCKS) return 0;
  if (workspace_bytes < (size_t)n_blocks * sizeof(int32_t)) return 0;
  return n_blocks;
}

// Count, scan, emit.  PINCH: the window rule, a compile-time mode like the two above; the default is the kernels that were.
template <bool STACK, int PINCH = GGNN_PINCH_JUNCTION>
static int launch_junctions(const ggnn::junction_kargs& K, int64_t n_blocks, int32_t boundary, hipStream_t st) {
  using namespace ggnn;
  const bool periodic = boundary == GGNN_BC_PERIODIC;
  const auto count = periodic ? image_junctions_kernel<false, GGNN_BC_PERIODIC, STACK, PINCH>
                              : image_junctions_kernel<false, GGNN_BC_NOFLUX, STACK, PINCH>;
  const auto emit = periodic ? image_junctions_kernel<true, GGNN_BC_PERIODIC, STACK, PINCH>
                             : image_junctions_kernel<true, GGNN_BC_NOFLUX, STACK, PINCH>;
  hipLaunchKernelGGL(count, dim3((unsigned)n_blocks), dim3(VEC_BLOCK), 0, st, K);
  hipLaunchKernelGGL(junction_scan_kernel<STACK>, dim3(1), dim3(VEC_SCAN_BLOCK), 0, st, K, (int64_t)(periodic ? 0 : 1));
  hipLaunchKernelGGL(emit, dim3((unsigned)n_blocks), dim3(VEC_BLOCK), 0, st, K);
  return launch_status();
}

extern "C" int ggnn_image_junctions(const ggnn_junction_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_junction_args& A = *args;
  junction_kargs K{A.image, nullptr, const_cast<uint64_t*>(A.pixel_counts), A.xy, A.triples, A.edge_gj, A.status, A.workspace,
                   nullptr, A.nx, A.ny, 1, A.n_grain, A.joint_capacity, A.offset, A.pitch, A.merge_radius, 0, 0, nullptr};
  const int64_t n_blocks = junction_blocks(K, A.workspace_bytes, A.boundary);
  if (!n_blocks) return GGNN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(A.status, 0, GGNN_JUNCTION_STATUS_WORDS * sizeof(int64_t), st) != hipSuccess) return GGNN_ELAUNCH;
  return launch_junctions<false>(K, n_blocks, A.boundary, st);
}

// ggnn_image_junctions_traj (rep NULL) and ggnn_image_junction_windows_traj: the same checks, the same launches.  Their
// _pinch twins come here with a mode and their counters, which take one memset more; GGNN_PINCH_NECK runs its own kernels.
static int image_junctions_traj(const ggnn_junction_traj_args* args, int32_t* rep, ggnn_stream_t stream,
                                int32_t pinch = GGNN_PINCH_JUNCTION, int64_t* pinch_windows = nullptr) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_junction_traj_args& A = *args;
  if (!A.grain_off || (reinterpret_cast<uintptr_t>(A.grain_off) & 7u)) return GGNN_EINVAL;
  junction_kargs K{A.images, A.grain_off, A.pixel_counts, A.xy, A.triples, A.edge_gj, A.status, A.workspace,
                   rep, A.nx, A.ny, A.n_image, A.n_grain, A.joint_capacity, A.offset, A.pitch, A.merge_radius, 0, 0, pinch_windows};
  const int64_t n_blocks = junction_blocks(K, A.workspace_bytes, A.boundary);
  if (!n_blocks) return GGNN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(A.status, 0, (size_t)A.n_image * GGNN_JUNCTION_STATUS_WORDS * sizeof(int64_t), st) != hipSuccess)
    return GGNN_ELAUNCH;
  if (hipMemsetAsync(A.pixel_counts, 0, (size_t)A.n_grain * sizeof(uint64_t), st) != hipSuccess) return GGNN_ELAUNCH;
  if (pinch_windows && hipMemsetAsync(pinch_windows, 0, (size_t)A.n_image * sizeof(int64_t), st) != hipSuccess) return GGNN_ELAUNCH;
  if (pinch == GGNN_PINCH_NECK) return launch_junctions<true, GGNN_PINCH_NECK>(K, n_blocks, A.boundary, st);
  return launch_junctions<true>(K, n_blocks, A.boundary, st);
}

// The checks the two _pinch twins add: a known mode comes with counters, 8-byte aligned.
static bool pinch_valid(int32_t pinch, const int64_t* pinch_windows) {
  if (pinch != GGNN_PINCH_JUNCTION && pinch != GGNN_PINCH_NECK) return false;
  return pinch_windows && !(reinterpret_cast<uintptr_t>(pinch_windows) & 7u);
}

extern "C" int ggnn_image_junctions_pinch_traj(const ggnn_junction_traj_args* args, int32_t pinch, int64_t* n_pinch_windows,
                                               ggnn_stream_t stream) {
  if (!pinch_valid(pinch, n_pinch_windows)) return GGNN_EINVAL;
  return image_junctions_traj(args, nullptr, stream, pinch, n_pinch_windows);
}

extern "C" int ggnn_image_junction_windows_pinch_traj(const ggnn_junction_traj_args* args, int32_t* rep, int32_t pinch,
                                                      int64_t* n_pinch_windows, ggnn_stream_t stream) {
  if (!rep || !pinch_valid(pinch, n_pinch_windows)) return GGNN_EINVAL;
  return image_junctions_traj(args, rep, stream, pinch, n_pinch_windows);
}

extern "C" int ggnn_image_junctions_traj(const ggnn_junction_traj_args* args, ggnn_stream_t stream) {
  return image_junctions_traj(args, nullptr, stream);
}

extern "C" int ggnn_image_junction_windows_traj(const ggnn_junction_traj_args* args, int32_t* rep, ggnn_stream_t stream) {
  if (!rep) return GGNN_EINVAL;
  return image_junctions_traj(args, rep, stream);
}

// The checks the two links entry points share (n_image: 1 for a single image).
static bool links_valid(const ggnn_link_traj_args& K) {
  if (!K.triples || !K.rowptr || !K.col || !K.edge_jj || !K.status) return false;
  if (K.n_grain < 1 || K.n_grain >= INT32_MAX - 1 || K.E_cap < 0 || K.E_cap >= INT32_MAX) return false;
  if (K.joint_capacity < 1 || K.joint_capacity > INT32_MAX / 3) return false;
  if (K.n_image < 1 || K.n_image > GGNN_JUNCTION_MAX_BLOCKS) return false;
  return !((reinterpret_cast<uintptr_t>(K.status) | reinterpret_cast<uintptr_t>(K.edge_jj)) & 7u);
}

extern "C" int ggnn_junction_links(const ggnn_link_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_link_args& A = *args;
  const ggnn_link_traj_args K{A.triples, A.rowptr, A.col, A.edge_jj, A.status, A.n_grain, A.joint_capacity, A.E_cap, 1};
  if (!links_valid(K)) return GGNN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(A.status + 4, 0, sizeof(int64_t), st) != hipSuccess) return GGNN_ELAUNCH;
  const int64_t blocks = (3 * A.joint_capacity + 255) / 256;
  hipLaunchKernelGGL(junction_links_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, K);
  return launch_status();
}

extern "C" int ggnn_junction_links_traj(const ggnn_link_traj_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_link_traj_args& A = *args;
  if (!links_valid(A)) return GGNN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(zero_open_pairs_kernel, dim3((unsigned)((A.n_image + 255) / 256)), dim3(256), 0, st, A.status, A.n_image);
  const int64_t blocks = (3 * A.joint_capacity + 255) / 256;
  hipLaunchKernelGGL(junction_links_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, A);
  return launch_status();
}

// ggnn_junction_links_trace_traj and its _pinch twin: the same checks, the same memset and launch.
static int junction_links_trace(const ggnn_link_trace_args* args, int32_t pinch, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  if (pinch != GGNN_PINCH_JUNCTION && pinch != GGNN_PINCH_NECK) return GGNN_EINVAL;
  const ggnn_link_trace_args& A = *args;
  if (!A.images || !A.grain_off || !A.triples || !A.rep || !A.rowptr || !A.col || !A.edge_jj || !A.status || !A.counters)
    return GGNN_EINVAL;
  if (A.n_grain < 1 || A.n_grain >= INT32_MAX - 1 || A.E_cap < 0 || A.E_cap >= INT32_MAX) return GGNN_EINVAL;
  if (A.joint_capacity < 1 || A.joint_capacity > INT32_MAX / 3) return GGNN_EINVAL;
  if (A.n_image < 1 || A.n_image > GGNN_JUNCTION_MAX_BLOCKS) return GGNN_EINVAL;
  if (A.merge_radius < 0 || A.merge_radius > VEC_MAX_RADIUS) return GGNN_EINVAL;
  if (A.nx <= 2 * A.merge_radius || A.ny <= 2 * A.merge_radius || A.nx >= (1 << 15) || A.ny >= (1 << 15)) return GGNN_EINVAL;
  if (A.boundary != GGNN_BC_PERIODIC && A.boundary != GGNN_BC_NOFLUX) return GGNN_EINVAL;
  if (A.max_trace < 1) return GGNN_EINVAL;
  if ((reinterpret_cast<uintptr_t>(A.status) | reinterpret_cast<uintptr_t>(A.edge_jj) | reinterpret_cast<uintptr_t>(A.counters) |
       reinterpret_cast<uintptr_t>(A.grain_off)) & 7u)
    return GGNN_EINVAL;
  if ((reinterpret_cast<uintptr_t>(A.images) | reinterpret_cast<uintptr_t>(A.triples) | reinterpret_cast<uintptr_t>(A.rep) |
       reinterpret_cast<uintptr_t>(A.rowptr) | reinterpret_cast<uintptr_t>(A.col)) & 3u)
    return GGNN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(A.counters, 0, (size_t)A.n_image * GGNN_TRACE_COUNTERS * sizeof(int64_t), st) != hipSuccess)
    return GGNN_ELAUNCH;
  const int64_t blocks = (3 * A.joint_capacity + 255) / 256;
  const bool periodic = A.boundary == GGNN_BC_PERIODIC;
  auto trace = periodic ? junction_trace_kernel<GGNN_BC_PERIODIC> : junction_trace_kernel<GGNN_BC_NOFLUX>;
  if (pinch == GGNN_PINCH_NECK)
    trace = periodic ? junction_trace_kernel<GGNN_BC_PERIODIC, GGNN_PINCH_NECK> : junction_trace_kernel<GGNN_BC_NOFLUX, GGNN_PINCH_NECK>;
  hipLaunchKernelGGL(trace, dim3((unsigned)blocks), dim3(256), 0, st, A);
  return launch_status();
}

extern "C" int ggnn_junction_links_trace_traj(const ggnn_link_trace_args* args, ggnn_stream_t stream) {
  return junction_links_trace(args, GGNN_PINCH_JUNCTION, stream);
}

extern "C" int ggnn_junction_links_trace_pinch_traj(const ggnn_link_trace_args* args, int32_t pinch, ggnn_stream_t stream) {
  return junction_links_trace(args, pinch, stream);
}
