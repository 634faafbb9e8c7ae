// Grain ids that persist across a sequence of labelled maps: the grains of consecutive frames are linked by their pixel overlap
// and the whole stack is renumbered.  The rule is include/ggnn.h's (ggnn_link_labels), restated by tests/linkcheck.py;
// everything here is exact in integers.
//
//   votes     a thread GGNN_LINK_RUN consecutive pixels of a row of a pair of frames: equal consecutive (b, a) pairs merged, one
//             bounded probe of the GGNN_LINK_SLOTS slots of (t, b) a distinct pair (atomicCAS on the key, atomicAdd on the count)
//   match     a thread a (t, b): the slots, the gates, the argmax; a 64-bit atomicMax on the claim word of (t - 1, a)
//   resolve   a thread a (t, b): pred stays only if the claim word names b; n_split, n_gone; the rows beyond a frame's grains
//   compose   one workgroup, t = 0 .. T - 1 in order over grain rows: a block scan of the fresh flags in chunks, the global ids,
//             first_frame, last_frame, theta, n_global
//   relabel   a thread a pixel
//
// No kernel waits on another workgroup: the order between workgroups is the order of the launches.  Every loop is bounded by T,
// local_capacity or the pixels.  Every id read from an image and every n_local read from the device is clamped before it
// indexes anything, and counted.  Which slot a key lands in depends on the order of the atomics; nothing that is written out does:
// the match reads all the slots of a grain and breaks ties by the ids.
#include <algorithm>

#include "common.h"

namespace ggnn {

constexpr int LINK_SLOTS = GGNN_LINK_SLOTS, LINK_RUN = GGNN_LINK_RUN, LINK_BLOCK = 256, LINK_COMPOSE_BLOCK = 1024;
enum { LK_LOCAL, LK_MATCHED, LK_FRESH, LK_SPLIT, LK_GONE, LK_VOTE_OVERFLOW };
static_assert(LK_VOTE_OVERFLOW + 1 == GGNN_LINK_FRAME_WORDS, "the per-frame status words of include/ggnn.h");
static_assert((LINK_SLOTS & (LINK_SLOTS - 1)) == 0, "the probe wraps with a mask");

struct LinkWs {             // the carved workspace
  int32_t* keys;            // [(T - 1) Lc SLOTS]: -1 empty, else the local id a of frame t - 1; frame t >= 1 at (t - 1) Lc SLOTS
  uint32_t* counts;         // [(T - 1) Lc SLOTS]
  unsigned long long* claim;   // [T Lc]: row a - first of frame t - 1, claimed by the grains of frame t (the last frame's: spare)
};
constexpr size_t LINK_ALIGN = 256;
static inline size_t link_up(size_t b) { return (b + LINK_ALIGN - 1) / LINK_ALIGN * LINK_ALIGN; }
static size_t link_carve(LinkWs* w, char* base, int64_t T, int64_t Lc, size_t* zero_from) {
  const size_t slots = (size_t)(T - 1) * (size_t)Lc * LINK_SLOTS;
  const size_t keys = link_up(4 * slots), counts = link_up(4 * slots), claim = link_up(8 * (size_t)T * (size_t)Lc);
  if (w) *w = LinkWs{(int32_t*)base, (uint32_t*)(base + keys), (unsigned long long*)(base + keys + counts)};
  if (zero_from) *zero_from = keys;                     // the keys are set to -1, everything behind them to 0
  return keys + counts + claim;
}

struct LinkDims {
  int64_t T, N, Lc, Gc;
  int nx, ny, K, first;
};

// the local grains of frame t: n_local[t] clamped to the rows there are
__device__ __forceinline__ int link_local(const int64_t* __restrict__ n_local, int64_t t, int64_t Lc) {
  const int64_t n = n_local[t];
  return (int)(n < 0 ? 0 : n > Lc ? Lc : n);
}

__device__ __forceinline__ void link_count_to(int64_t* word, unsigned long long v) {   // a sum over the wave, one atomic
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long*)word, v);
}

// ---- votes -------------------------------------------------------------------------------------------------------------------
// `n` pixels hold b in frame t and a in frame t - 1, both local grains (row indices rb < L_t, ra < L_(t-1)) -> false: dropped
__device__ __forceinline__ bool link_vote(const LinkWs& W, const LinkDims& D, int64_t t, int rb, int ra, unsigned n) {
  const int64_t base = ((t - 1) * D.Lc + rb) * LINK_SLOTS;
  const unsigned h = ((unsigned)ra * 2654435761u) >> 28;
  for (int s = 0; s < LINK_SLOTS; ++s) {
    const int64_t at = base + ((h + s) & (LINK_SLOTS - 1));
    const int seen = atomicCAS(W.keys + at, -1, ra);
    if (seen == -1 || seen == ra) {
      atomicAdd(W.counts + at, n);
      return true;
    }
  }
  return false;
}

__global__ __launch_bounds__(LINK_BLOCK) void link_votes_kernel(const int32_t* __restrict__ labels, const int64_t* __restrict__ n_local,
                                                                LinkWs W, int64_t* __restrict__ status, LinkDims D) {
  const int64_t runs_x = (D.nx + LINK_RUN - 1) / LINK_RUN, runs_frame = runs_x * D.ny, runs = runs_frame * (D.T - 1);
  for (int64_t r = (int64_t)blockIdx.x * LINK_BLOCK + threadIdx.x; r < runs; r += (int64_t)gridDim.x * LINK_BLOCK) {
    const int64_t t = 1 + r / runs_frame, in_frame = r % runs_frame;
    const int y = (int)(in_frame / runs_x), x0 = (int)(in_frame % runs_x) * LINK_RUN;
    const int La = link_local(n_local, t - 1, D.Lc), Lb = link_local(n_local, t, D.Lc);
    const int32_t* cur = labels + t * D.N + (int64_t)y * D.nx;
    const int32_t* before = cur - D.N;
    int rb = -1, ra = -1;
    unsigned n = 0, dropped = 0;
    for (int j = 0; j < LINK_RUN; ++j) {
      const int x = x0 + j;
      int qb = -1, qa = -1;
      if (x < D.nx) {
        const int64_t b = (int64_t)cur[x] - D.first, a = (int64_t)before[x] - D.first;
        if (b >= 0 && b < Lb && a >= 0 && a < La) qb = (int)b, qa = (int)a;
      }
      if (qb == rb && qa == ra) {
        ++n;
        continue;
      }
      if (rb >= 0 && !link_vote(W, D, t, rb, ra, n)) dropped += n;
      rb = qb, ra = qa, n = 1;
    }
    if (rb >= 0 && !link_vote(W, D, t, rb, ra, n)) dropped += n;
    if (dropped) atomicAdd((unsigned long long*)(status + t * GGNN_LINK_FRAME_WORDS + LK_VOTE_OVERFLOW), (unsigned long long)dropped);
  }
}

// ---- match, resolve: a block works on one frame (blockIdx.y strides the frames) ------------------------------------------------
__global__ __launch_bounds__(LINK_BLOCK) void link_match_kernel(const int64_t* __restrict__ n_local, const float* __restrict__ means, LinkWs W,
                                                                int32_t* __restrict__ pred, LinkDims D, int64_t min_overlap, float match_tol,
                                                                int gate) {
  for (int64_t t = 1 + blockIdx.y; t < D.T; t += gridDim.y) {
    const int Lb = link_local(n_local, t, D.Lc), La = link_local(n_local, t - 1, D.Lc);
    for (int64_t i = (int64_t)blockIdx.x * LINK_BLOCK + threadIdx.x; i < Lb; i += (int64_t)gridDim.x * LINK_BLOCK) {
      const int64_t base = ((t - 1) * D.Lc + i) * LINK_SLOTS;
      int best = -1;
      unsigned best_n = 0;
      for (int s = 0; s < LINK_SLOTS; ++s) {
        const int ra = W.keys[base + s];
        const unsigned n = W.counts[base + s];
        if (ra < 0 || ra >= La || (int64_t)n < min_overlap) continue;
        bool alike = true;
        if (gate)
          for (int k = 0; k < D.K; ++k)
            alike &= fabsf(__fsub_rn(means[(t * D.K + k) * D.Lc + i], means[((t - 1) * D.K + k) * D.Lc + ra])) <= match_tol;
        if (alike && (n > best_n || (n == best_n && ra < best))) best = ra, best_n = n;
      }
      pred[t * D.Lc + i] = best < 0 ? -1 : best + D.first;
      if (best >= 0)
        atomicMax(W.claim + (t - 1) * D.Lc + best, ((unsigned long long)best_n << 32) | (0xFFFFFFFFull - (unsigned long long)i));
    }
  }
}

__global__ __launch_bounds__(LINK_BLOCK) void link_resolve_kernel(const int64_t* __restrict__ n_local, LinkWs W, int32_t* __restrict__ gid,
                                                                  int32_t* __restrict__ pred, int64_t* __restrict__ status, LinkDims D) {
  for (int64_t t = blockIdx.y; t < D.T; t += gridDim.y) {
    const int Lb = link_local(n_local, t, D.Lc), La = t > 0 ? link_local(n_local, t - 1, D.Lc) : 0;
    unsigned long long split = 0, gone = 0;
    for (int64_t i = (int64_t)blockIdx.x * LINK_BLOCK + threadIdx.x; i < D.Lc; i += (int64_t)gridDim.x * LINK_BLOCK) {
      if (i >= Lb) {
        gid[t * D.Lc + i] = 0;
        pred[t * D.Lc + i] = -1;
      } else if (t == 0) {
        pred[i] = -1;
      } else {
        const int a = pred[t * D.Lc + i] - D.first;
        if (a >= 0 && a < La && (uint32_t)W.claim[(t - 1) * D.Lc + a] != 0xFFFFFFFFu - (uint32_t)i) {
          pred[t * D.Lc + i] = -1;
          ++split;
        }
      }
      if (i < La && W.claim[(t - 1) * D.Lc + i] == 0) ++gone;       // (a claim carries a vote of at least 1: never 0)
    }
    link_count_to(status + t * GGNN_LINK_FRAME_WORDS + LK_SPLIT, split);
    link_count_to(status + t * GGNN_LINK_FRAME_WORDS + LK_GONE, gone);
  }
}

// ---- compose: one workgroup, the frames in order -----------------------------------------------------------------------------------
__device__ __forceinline__ int link_block_exclusive(int mine, int* total, int* wave_sums) {   // LINK_COMPOSE_BLOCK threads, 16 waves
  constexpr int WAVES = LINK_COMPOSE_BLOCK / 64;
  int incl = mine;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wave_sums[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < WAVES; ++w) {
    before += w < wave ? wave_sums[w] : 0;
    all += wave_sums[w];
  }
  *total = all;
  __syncthreads();
  return before + incl - mine;
}

__global__ __launch_bounds__(LINK_COMPOSE_BLOCK) void link_compose_kernel(const int64_t* __restrict__ n_local, const float* __restrict__ means,
                                                                          const int32_t* __restrict__ pred, int32_t* gid,
                                                                          int32_t* __restrict__ first_frame, int32_t* __restrict__ last_frame,
                                                                          float* __restrict__ theta, int64_t* __restrict__ status, LinkDims D) {
  __shared__ int wave_sums[LINK_COMPOSE_BLOCK / 64];
  const int L0 = link_local(n_local, 0, D.Lc);
  int64_t n_global = L0, bad_frames = 0;
  for (int64_t t = 0; t < D.T; ++t) {
    const int L = link_local(n_local, t, D.Lc), Lp = t > 0 ? link_local(n_local, t - 1, D.Lc) : 0;
    bad_frames += n_local[t] < 0 || n_local[t] > D.Lc;
    int64_t fresh_in_frame = 0;
    for (int i0 = 0; i0 < L; i0 += LINK_COMPOSE_BLOCK) {             // (L <= local_capacity < 2^31)
      const int i = i0 + (int)threadIdx.x;
      const int a = i < L && t > 0 ? pred[t * D.Lc + i] - D.first : -1;
      const bool kept = a >= 0 && a < Lp, fresh = i < L && t > 0 && !kept;
      int total;
      const int before = link_block_exclusive(fresh, &total, wave_sums);
      if (i < L) {
        // (gid of frame t - 1: written by this workgroup before the barriers above)
        const int64_t g = t == 0 ? i : fresh ? n_global + before : (int64_t)gid[(t - 1) * D.Lc + a] - D.first;
        gid[t * D.Lc + i] = (int32_t)(g + D.first);
        if (g >= 0 && g < D.Gc) {
          last_frame[g] = (int32_t)t;
          if (t == 0 || fresh) {
            first_frame[g] = (int32_t)t;
            for (int k = 0; k < D.K; ++k) theta[k * D.Gc + g] = means[(t * D.K + k) * D.Lc + i];
          }
        }
      }
      n_global += total;
      fresh_in_frame += total;
    }
    __syncthreads();                                                  // frame t's ids before frame t + 1 reads them
    if (threadIdx.x == 0) {
      int64_t* s = status + t * GGNN_LINK_FRAME_WORDS;
      s[LK_LOCAL] = L;
      s[LK_FRESH] = fresh_in_frame;
      s[LK_MATCHED] = t > 0 ? L - fresh_in_frame : 0;
    }
  }
  if (threadIdx.x == 0) {
    status[D.T * GGNN_LINK_FRAME_WORDS] = n_global;
    const unsigned long long over = (unsigned long long)bad_frames + (n_global > D.Gc ? 1 : 0);
    if (over) atomicAdd((unsigned long long*)(status + D.T * GGNN_LINK_FRAME_WORDS + 1), over);
  }
}

// ---- relabel -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LINK_BLOCK) void link_relabel_kernel(const int32_t* __restrict__ labels, const int64_t* __restrict__ n_local,
                                                                  const int32_t* __restrict__ gid, int32_t* __restrict__ out,
                                                                  int64_t* __restrict__ status, LinkDims D) {
  const int64_t all = D.T * D.N;
  unsigned long long outside = 0;
  for (int64_t p = (int64_t)blockIdx.x * LINK_BLOCK + threadIdx.x; p < all; p += (int64_t)gridDim.x * LINK_BLOCK) {
    const int64_t t = p / D.N;
    const int32_t b = labels[p];
    const int64_t row = (int64_t)b - D.first;
    int32_t g = 0;
    if (row >= 0 && row < link_local(n_local, t, D.Lc))
      g = gid[t * D.Lc + row];
    else if (b == 1 && D.first == 2)
      g = 1;                                                          // the boundary grain of a no-flux image
    else if (b != 0)
      ++outside;
    out[p] = g;
  }
  link_count_to(status + D.T * GGNN_LINK_FRAME_WORDS + 1, outside);
}

static inline bool link_sizes_ok(int64_t T, int64_t Lc, int32_t K) {
  return T >= 1 && Lc >= 1 && Lc < INT32_MAX && K >= 0 && K <= 4 && T <= (1ll << 36) / Lc;
}

}  // namespace ggnn

extern "C" size_t ggnn_link_workspace_bytes(int64_t T, int64_t local_capacity, int32_t K) {
  if (!ggnn::link_sizes_ok(T, local_capacity, K)) return 0;
  return ggnn::link_carve(nullptr, nullptr, T, local_capacity, nullptr);
}

extern "C" int ggnn_link_labels(const ggnn_link_labels_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_link_labels_args& A = *args;
  if (!A.labels || !A.n_local || !A.frames_out || !A.gid || !A.pred || !A.first_frame || !A.last_frame || !A.status || !A.workspace)
    return GGNN_EINVAL;
  if (!link_sizes_ok(A.T, A.local_capacity, A.K) || A.global_capacity < 1 || A.global_capacity >= INT32_MAX) return GGNN_EINVAL;
  if (A.nx < 3 || A.ny < 3 || A.nx >= (1 << 15) || A.ny >= (1 << 15)) return GGNN_EINVAL;
  if (A.K > 0 && (!A.means || !A.theta)) return GGNN_EINVAL;
  if (A.min_overlap < 1 || (A.use_match_tol && (A.K == 0 || !(A.match_tol >= 0.0f)))) return GGNN_EINVAL;
  if (A.boundary != GGNN_BC_PERIODIC && A.boundary != GGNN_BC_NOFLUX) return GGNN_EINVAL;
  auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
  if ((at(A.n_local) & 7u) || (at(A.status) & 7u) || (at(A.workspace) & 7u) || (at(A.labels) & 3u) || (at(A.means) & 3u) ||
      (at(A.frames_out) & 3u) || (at(A.gid) & 3u) || (at(A.pred) & 3u) || (at(A.first_frame) & 3u) || (at(A.last_frame) & 3u) ||
      (at(A.theta) & 3u))
    return GGNN_EINVAL;
  LinkWs W;
  size_t zero_from;
  const size_t need = link_carve(&W, (char*)A.workspace, A.T, A.local_capacity, &zero_from);
  if (A.workspace_bytes < need) return GGNN_EINVAL;
  const LinkDims D{A.T, A.nx * A.ny, A.local_capacity, A.global_capacity, (int)A.nx, (int)A.ny, A.K, A.boundary == GGNN_BC_PERIODIC ? 1 : 2};
  hipStream_t st = (hipStream_t)stream;
  const size_t status_bytes = (size_t)(A.T * GGNN_LINK_FRAME_WORDS + GGNN_LINK_GLOBAL_WORDS) * sizeof(int64_t);
  bool ok = hipMemsetAsync(A.status, 0, status_bytes, st) == hipSuccess;
  if (zero_from) ok = ok && hipMemsetAsync(W.keys, 0xFF, zero_from, st) == hipSuccess;
  ok = ok && hipMemsetAsync((char*)A.workspace + zero_from, 0, need - zero_from, st) == hipSuccess;
  ok = ok && hipMemsetAsync(A.first_frame, 0xFF, (size_t)A.global_capacity * sizeof(int32_t), st) == hipSuccess;
  ok = ok && hipMemsetAsync(A.last_frame, 0xFF, (size_t)A.global_capacity * sizeof(int32_t), st) == hipSuccess;
  if (A.K > 0) ok = ok && hipMemsetAsync(A.theta, 0, (size_t)A.K * (size_t)A.global_capacity * sizeof(float), st) == hipSuccess;
  if (!ok) return GGNN_ELAUNCH;
  const int64_t wide_cap = 16 * (int64_t)num_cu();
  auto blocks = [&](int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + LINK_BLOCK - 1) / LINK_BLOCK, wide_cap)); };
  const dim3 block(LINK_BLOCK);
  const unsigned rows_x = blocks(A.local_capacity);
  if (A.T > 1) {
    const int64_t runs = (A.nx + LINK_RUN - 1) / LINK_RUN * A.ny * (A.T - 1);
    hipLaunchKernelGGL(link_votes_kernel, dim3(blocks(runs)), block, 0, st, A.labels, A.n_local, W, A.status, D);
    hipLaunchKernelGGL(link_match_kernel, dim3(rows_x, (unsigned)std::min<int64_t>(A.T - 1, 1024)), block, 0, st, A.n_local, A.means, W, A.pred, D,
                       A.min_overlap, A.match_tol, A.use_match_tol ? 1 : 0);
  }
  hipLaunchKernelGGL(link_resolve_kernel, dim3(rows_x, (unsigned)std::min<int64_t>(A.T, 1024)), block, 0, st, A.n_local, W, A.gid, A.pred, A.status,
                     D);
  hipLaunchKernelGGL(link_compose_kernel, dim3(1), dim3(LINK_COMPOSE_BLOCK), 0, st, A.n_local, A.means, A.pred, A.gid, A.first_frame,
                     A.last_frame, A.theta, A.status, D);
  hipLaunchKernelGGL(link_relabel_kernel, dim3(blocks(D.T * D.N)), block, 0, st, A.labels, A.n_local, A.gid, A.frames_out, A.status, D);
  return launch_status();
}
