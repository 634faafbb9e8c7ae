// Rollout-step glue on device (static topology):
//   ggnn_step_update  = GrainNN_regressor.update, periodic branch (models.py:503-516)
//                       + z advance (test.py:401-402)
//   ggnn_step_refresh = z clamp (test.py:405-407) + edge-length refresh (test.py:562-575)
//   ggnn_noflux_boundary[_traj] = the no-flux boundary step (test.py:446-463), after the topology update
//   ggnn_process_schedule = the (G, R) features of the step to come (test.py:376-379), row by a device-side counter
//   ggnn_grain_centres = region centres of graph.update() (graph_datastruct.py:681-708) written
//                       to x_grain[:, :2] (test.py:468-478, 556-559), between the two
// Separate launches because each stage needs every node's updated coordinates.
#include "common.h"
#include "segments.h"

namespace ggnn {

__global__ __launch_bounds__(256) void step_update_kernel(
    float* __restrict__ x_joint, int64_t n_joint, int64_t ldxj, float* __restrict__ x_grain,
    int64_t n_grain, int64_t ldxg, int f_grain, const float* __restrict__ y_joint,
    const float* __restrict__ y_grain, float dz, float zmax, int32_t* __restrict__ flags) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n_joint) {
    float* x = x_joint + t * ldxj;
    const float dx = y_joint[2 * t], dy = y_joint[2 * t + 1];
    x[0] += dx / 5.0f;  // models.py:505 (scaling['joint'] = 5)
    x[1] += dy / 5.0f;
    x[2] += dz;         // test.py:402
    x[6] = dx;          // models.py:510
    x[7] = dy;
  } else if (t < n_joint + n_grain) {
    const int64_t g = t - n_joint;
    float* x = x_grain + g * ldxg;
    const float da = y_grain[2 * g], dv = y_grain[2 * g + 1];
    const float z = x[2] + dz;  // test.py:401
    x[2] = z;
    x[3] += da / 20.0f;  // models.py:506 (scaling['grain'] = 20)
    x[4] = dv;           // :507
    x[f_grain - 1] = da;  // :511
    if (g == 0) flags[1] = z > zmax ? 1 : 0;  // test.py:405
  }
}

// One thread per grain: walk the grain's junctions (CSR row of the joint->grain edge type),
// min-image each to the previous moved one, shift by +1 where any vertex is below -eps, mean.
// ~6 junctions x 8 B per grain: the launch is latency-, not bandwidth-bound.
// PERIODIC = false: the no-flux branch (graph_datastruct.py:689-692), no min-image chaining.
template <bool PERIODIC>
__global__ __launch_bounds__(256) void grain_centres_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const float* __restrict__ x_joint, int64_t ldxj, const float* __restrict__ offset,
    float factor, float* __restrict__ x_grain, int64_t ldxg, int64_t n_grain, int64_t n_joint,
    float* __restrict__ centres_before) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n_grain) return;
  if (centres_before != nullptr) {   // the centres as this call found them (the speculative event loop's snapshot)
    centres_before[2 * g] = x_grain[g * ldxg];
    centres_before[2 * g + 1] = x_grain[g * ldxg + 1];
  }
  const int p0 = rowptr[g], p1 = rowptr[g + 1];
  if (p1 - p0 <= 1) return;  // graph_datastruct.py:685: such a region keeps its centre
  const bool folded = factor > 1.0f;
  float prev[2], sum[2] = {0.f, 0.f}, lo[2] = {INFINITY, INFINITY};
  // batches of 8 junctions: the index loads, then the coordinate loads, are issued together; only
  // the min-image chain itself is sequential
  for (int q0 = p0; q0 < p1; q0 += 8) {
    int64_t js[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) js[k] = min((int64_t)max(col[min(q0 + k, p1 - 1)], 0), n_joint - 1);
    float raw[8][2];
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float t = x_joint[js[k] * ldxj + c];
        if (folded) t = (t + (offset ? offset[2 * js[k] + c] : 0.f)) / factor;  // test.py:474
        raw[k][c] = t;
      }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (q0 + k >= p1) break;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float t = raw[k][c];
        if (PERIODIC && q0 + k > p0) {  // periodic_move, graph_datastruct.py:55-72
          const float rel = t - prev[c];
          t += rel > 0.5f ? -1.0f : (rel < -0.5f ? 1.0f : 0.0f);
        }
        prev[c] = t;
        sum[c] += t;
        lo[c] = fminf(lo[c], t);
      }
    }
  }
  const float inv = 1.0f / (float)(p1 - p0);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float m = sum[c] * inv;
    if (!(lo[c] > -1e-12f)) m += 1.0f;  // inbound test, graph_datastruct.py:696-704
    if (folded) {                        // test.py:558-559
      m *= factor;
      m -= floorf(m);
    }
    x_grain[g * ldxg + c] = m;
  }
}

// What the kernel of both detection entry points takes, filled from their arguments.
struct detect_kargs {
  const float* __restrict__ grain_area;
  const int32_t* __restrict__ live_grain;
  const float* __restrict__ edge_event;
  const int64_t* __restrict__ ei_jj;
  const int64_t* __restrict__ E_dev;
  int32_t* __restrict__ flags;
  int32_t* __restrict__ range_word;
  int64_t n_grain, E_cap;
  float area_threshold, logit_threshold;
  int64_t skip_grain;                           // UNION = false alone
  const int64_t* __restrict__ traj_grain_off;   // UNION = true alone, from here on
  const int64_t* __restrict__ traj_joint_off;
  const int32_t* __restrict__ ended;
  int32_t* __restrict__ counts;
  int n_traj;
};

// Counts the events the host-side topology update would act on (test.py:418, models.py:624-626): the live grains with
// grain_area < area_threshold and the directed junction edges (src < dst) with edge_event > logit_threshold.  One pass over
// 10k + 60k values; the rollout reads the words back once per step and only touches the host path when one is non-zero.
// UNION = false: flags[0] += the grains (skip_grain left out), flags[1] += the edges, a ballot and an atomic a wave each.
// UNION = true, a disjoint union of trajectories: the same candidates, counted per trajectory as well.  A grain
// belongs to the trajectory whose range of traj_grain_off holds it, a junction edge to the trajectory of its source junction;
// the boundaries fall anywhere inside a wave.  Candidates are rare: a block without one leaves at once; one with candidates
// stages the offsets in LDS while they fit (DET_LDS_TRAJ) and only its candidate lanes search them.  A wave's candidates of
// one (trajectory, kind) go out as one pair of integer atomics: exact and order-free.
constexpr int DET_LDS_TRAJ = 511;   // 2 x 512 offsets of 8 bytes: 8 KiB
template <bool UNION>
__global__ __launch_bounds__(256) void detect_events_kernel(const detect_kargs A) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t E = A.E_dev ? *A.E_dev : A.E_cap;   // (E_dev: include/ggnn.h, ggnn_prepare_edge)
  // (the caller's fp16-range word travels with the counts and starts its next use clean: one thread moves it)
  if (A.range_word != nullptr && t == 0) A.flags[2] = atomicExch(A.range_word, 0);
  bool cand = false;
  int kind = 0;       // 0: grain, 1: junction edge
  int64_t node = 0;   // the grain, or the edge's source junction
  if (t < A.n_grain) {
    cand = (UNION || t != A.skip_grain) && A.live_grain[t] > 0 && A.grain_area[t] < A.area_threshold;
    node = t;
  } else if (t - A.n_grain < E) {
    const int64_t k = t - A.n_grain;
    kind = 1;
    if (A.edge_event[k] > A.logit_threshold) {
      node = A.ei_jj[k];
      cand = node < A.ei_jj[E + k];
    }
  }
  if constexpr (!UNION) {
    const int ng = __popcll(__ballot(cand && kind == 0)), ne = __popcll(__ballot(cand && kind == 1));
    if ((threadIdx.x & 63) == 0) {
      if (ng) atomicAdd(&A.flags[0], ng);
      if (ne) atomicAdd(&A.flags[1], ne);
    }
  } else {
    __shared__ int64_t s_off[2][DET_LDS_TRAJ + 1];
    if (!__syncthreads_or(cand)) return;   // (uniform over the block: nobody waits at the barrier below)
    const bool staged = A.n_traj <= DET_LDS_TRAJ;
    if (staged) {
      for (int i = threadIdx.x; i <= A.n_traj; i += 256) {
        s_off[0][i] = A.traj_grain_off[i];
        s_off[1][i] = A.traj_joint_off[i];
      }
      __syncthreads();
    }
    int key = 0;   // 2 x trajectory + kind: the candidate's word of counts [n_traj, 2]
    if (cand) {
      const int tr = seg_of(staged ? s_off[kind] : (kind ? A.traj_joint_off : A.traj_grain_off), A.n_traj, node);
      if (A.ended != nullptr && A.ended[tr] != 0) cand = false;
      key = 2 * tr + kind;
    }
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(cand);
    while (todo) {   // (wave-uniform)
      const int lead = __ffsll(todo) - 1;
      const int lead_key = __shfl(key, lead);
      const unsigned long long same = __ballot(cand && key == lead_key);
      if (lane == lead) {
        const int n = __popcll(same);
        atomicAdd(&A.counts[lead_key], n);
        atomicAdd(&A.flags[lead_key & 1], n);
      }
      todo &= ~same;
    }
  }
}

// The no-flux boundary step (test.py:446-463): one thread per junction.  Whether a junction is one of its boundary grain's
// (that grain's row of the full joint->grain CSR, a few dozen to a few hundred junctions on the walls) is looked up in LDS,
// one chunk of the row at a time.  Every fp32 operation is rounded on its own, in the reference's order: torch evaluates
// (xy + off) / f and xy * f - off as separate ops, which a contraction into an fma would not reproduce.
// One rollout (traj_joint_off == nullptr): one trajectory, every junction, boundary grain 0.  A disjoint union of n_traj
// trajectories: trajectory t owns the junctions [traj_joint_off[t], traj_joint_off[t + 1]) and its boundary grain is its
// first one, traj_grain_off[t].  A block's 256 junctions span a contiguous range of trajectories, found once per block; the
// block walks that range -- a trip count that is uniform over the block, so that every thread reaches every barrier -- and
// stages each trajectory's boundary row, against which only that trajectory's lanes compare: a junction pays for the length
// of its own trajectory's row.  UNION = false compiles the same body without the walk: the single rollout's launch costs
// what it cost before unions.
constexpr int BND_CHUNK = 1024;
template <bool UNION>
__global__ __launch_bounds__(256) void noflux_boundary_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, float* __restrict__ x_joint, int64_t n_joint,
    int64_t ldxj, const float* __restrict__ offset, float factor, float max_y, float* __restrict__ x_grain, int64_t ldxg,
    int f_grain, float* __restrict__ joints_before, const int64_t* __restrict__ traj_grain_off,
    const int64_t* __restrict__ traj_joint_off, int n_traj) {
  __shared__ int32_t s_b[BND_CHUNK];
  const int64_t first = (int64_t)blockIdx.x * 256;
  const int64_t t = first + threadIdx.x;
  const bool live = t < n_joint;
  float xy[2] = {0.f, 0.f};
  if (live) {
    float* x = x_joint + t * ldxj;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float v = x[c];
      if (joints_before) joints_before[2 * t + c] = v;
      xy[c] = __fdiv_rn(offset ? __fadd_rn(v, offset[2 * t + c]) : v, factor);   // test.py:453
    }
  }
  // the trajectories of the block's first and last junction (block-uniform)
  int tr = 0, tr_last = 0;
  if (UNION) {
    tr = seg_of(traj_joint_off, n_traj, first);
    tr_last = seg_of(traj_joint_off, n_traj, min(first + 255, n_joint - 1));
  }
  bool bound = false;
  for (; tr <= tr_last; ++tr) {
    int64_t j0 = 0, j1 = n_joint, g0 = 0;
    if (UNION) {
      j0 = traj_joint_off[tr];
      j1 = traj_joint_off[tr + 1];
      g0 = traj_grain_off[tr];
    }
    if (j0 >= j1) continue;   // an empty trajectory inside the range (block-uniform)
    if (t == j0) {   // test.py:450-452, once per trajectory: by its first junction, wherever in a block that falls
      float* g = x_grain + g0 * ldxg;
      g[0] = 0.5f;
      g[1] = 0.5f;
      g[3] = 0.0f;
      g[4] = 0.0f;
      g[f_grain - 1] = 0.0f;
    }
    const bool mine = live && t >= j0 && t < j1;
    const int32_t b0 = rowptr[g0], b1 = rowptr[g0 + 1];
    for (int32_t q0 = b0; q0 < b1; q0 += BND_CHUNK) {   // (uniform trip count: every thread reaches the barriers)
      const int32_t nq = min(BND_CHUNK, b1 - q0);
      __syncthreads();
      for (int k = threadIdx.x; k < nq; k += 256) s_b[k] = col[q0 + k];
      __syncthreads();
      if (mine)
        for (int k = 0; k < nq; ++k) bound = bound || s_b[k] == (int32_t)t;
    }
  }
  if (!live) return;
  if (bound) {   // move_to_boundary, test.py:58-71: torch.argmin keeps the first of equal minima
    const float d[4] = {xy[0], __fsub_rn(1.0f, xy[0]), xy[1], __fsub_rn(max_y, xy[1])};
    int k = 0;
    float m = d[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
      if (d[i] < m) {
        m = d[i];
        k = i;
      }
    if (k == 0) xy[0] = 0.0f;
    else if (k == 1) xy[0] = 1.0f;
    else if (k == 2) xy[1] = 0.0f;
    else xy[1] = max_y;
  }
  const float hi[2] = {1.0f, max_y};   // test.py:461-462
  float* x = x_joint + t * ldxj;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float v = xy[c];
    v = v < 0.0f ? 0.0f : (v > hi[c] ? hi[c] : v);
    const float w = __fmul_rn(v, factor);   // test.py:466
    x[c] = offset ? __fsub_rn(w, offset[2 * t + c]) : w;
  }
}

// The process parameters of the step to come (test.py:376-379), from a table of feature values on the device: one thread per
// junction, two 4-byte stores (columns 3 and 4; a row's column 3 is not 8-byte aligned for every ldx).  The table's row
// follows a device-side counter, so that a captured graph replays with the counter where the replay before left it (the
// mechanism of the QoI layer counter, qoi.hip): every block reads the counter at its top, and the last block to finish -- by
// then every block has read it -- stores counter + 1, which may go to the same word.  A junction's trajectory is the last
// offset <= the junction (seg_of, segments.h); the offsets and the table's current row are staged in LDS while they fit
// (SCH_LDS_TRAJ), read from global memory beyond that; `staged` depends on kernel arguments only, so the barrier behind the
// staging is reached by every thread of every block or by none.
constexpr int SCH_LDS_TRAJ = 512;   // 513 offsets of 8 bytes + 512 rows of 8 bytes: 8 KiB
__global__ __launch_bounds__(256) void process_schedule_kernel(
    float* __restrict__ x_joint, int64_t n_joint, int64_t ldxj, const float* __restrict__ table, int64_t n_rows, int n_traj,
    const int64_t* __restrict__ traj_joint_off, const int32_t* step_in, int32_t* step_out, int32_t* sync_word) {
  __shared__ int64_t s_off[SCH_LDS_TRAJ + 1];
  __shared__ float s_row[2 * SCH_LDS_TRAJ];
  const int32_t k = *step_in;
  // the row of the step to come, inside the table for any counter: negative ones land on row 0, late ones on the last row
  const int64_t r = min(max((int64_t)k + 1, (int64_t)0), n_rows - 1);
  const float* row = table + r * (2 * (int64_t)n_traj);
  const bool staged = traj_joint_off != nullptr && n_traj <= SCH_LDS_TRAJ;
  if (staged) {
    for (int i = threadIdx.x; i <= n_traj; i += 256) s_off[i] = traj_joint_off[i];
    for (int i = threadIdx.x; i < 2 * n_traj; i += 256) s_row[i] = row[i];
    __syncthreads();
  }
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n_joint) {
    const int t = traj_joint_off == nullptr ? 0 : seg_of(staged ? s_off : traj_joint_off, n_traj, j);
    const float* v = staged ? s_row : row;
    float* x = x_joint + j * ldxj;
    x[3] = v[2 * t];
    x[4] = v[2 * t + 1];
  }
  // the last block to get here has seen every other block read the counter
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(sync_word, 1) == (int32_t)gridDim.x - 1) {
      *sync_word = 0;
      *step_out = k < INT32_MAX ? k + 1 : k;
    }
  }
}

struct RefreshArgs {
  ggnn_refresh_edge et[3];
  int64_t e_off[4];  // prefix sums of E over the edge types
  int n_et;
};

__global__ __launch_bounds__(256) void step_refresh_kernel(
    float* __restrict__ x_joint, int64_t n_joint, int64_t ldxj, float* __restrict__ x_grain,
    int64_t n_grain, int64_t ldxg, float zmax, const int32_t* __restrict__ flags,
    const RefreshArgs R) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n_nodes = n_joint + n_grain;
  if (t < n_nodes) {
    if (flags[1]) {  // test.py:405-407
      if (t < n_joint)
        x_joint[t * ldxj + 2] = zmax;
      else
        x_grain[(t - n_joint) * ldxg + 2] = zmax;
    }
    return;
  }
  const int64_t eg = t - n_nodes;
  if (eg >= R.e_off[R.n_et]) return;
  int k = 0;
  while (k + 1 < R.n_et && eg >= R.e_off[k + 1]) ++k;
  const ggnn_refresh_edge& T = R.et[k];
  const int64_t e = eg - R.e_off[k];
  const int64_t E = T.E_dev ? *T.E_dev : T.E;   // (E_dev: include/ggnn.h, ggnn_prepare_edge)
  if (e >= E) return;
  const int64_t s = T.edge_index[e], d = T.edge_index[E + e];
  if ((uint64_t)s >= (uint64_t)T.n_src || (uint64_t)d >= (uint64_t)T.n_dst) {
    T.edge_attr[e] = NAN;  // never reached for an edge_index that passed ggnn_build_csr_batch
    return;
  }
  const float* xs = T.x_src + s * T.ldx_src;
  const float* xd = T.x_dst + d * T.ldx_dst;
  float r[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {  // test.py:570-571
    const float rel = xs[c] - xd[c];
    const float w = rel > 0.5f ? -1.0f : (rel < -0.5f ? 1.0f : 0.0f);
    r[c] = w + rel;
  }
  T.edge_attr[e] = sqrtf(r[0] * r[0] + r[1] * r[1]);  // test.py:572
}

// ggnn_noflux_boundary (traj_joint_off NULL, n_traj 1) and ggnn_noflux_boundary_traj, which has checked its union arguments.
static int launch_noflux_boundary(const int32_t* rowptr_jg, const int32_t* col_jg, float* x_joint, int64_t n_joint,
                                  int64_t ldx_joint, const float* domain_offset, float domain_factor, float max_y,
                                  float* x_grain, int64_t ldx_grain, int f_grain, float* joints_before,
                                  const int64_t* traj_grain_off, const int64_t* traj_joint_off, int n_traj, hipStream_t stream) {
  if (!rowptr_jg || !col_jg || !x_joint || !x_grain || n_joint <= 0) return GGNN_EINVAL;
  if (ldx_joint < 2 || f_grain < 6 || ldx_grain < f_grain) return GGNN_EINVAL;
  if (!(domain_factor >= 1.0f) || !(max_y > 0.0f)) return GGNN_EINVAL;
  const int64_t nblk = (n_joint + 255) / 256;
  if (nblk >= INT32_MAX) return GGNN_EINVAL;
  hipLaunchKernelGGL(traj_joint_off ? noflux_boundary_kernel<true> : noflux_boundary_kernel<false>, dim3((unsigned)nblk),
                     dim3(256), 0, stream, rowptr_jg, col_jg, x_joint, n_joint, ldx_joint, domain_offset, domain_factor, max_y,
                     x_grain, ldx_grain, f_grain, joints_before, traj_grain_off, traj_joint_off, n_traj);
  return launch_status();
}

// Both detection entry points: the checks they share, the grid, the memsets of flags and -- a union -- of counts, the launch.
static int launch_detect_events(const detect_kargs& A, bool is_union, hipStream_t stream) {
  if (!A.grain_area || !A.live_grain || !A.flags || A.n_grain <= 0 || A.E_cap < 0) return GGNN_EINVAL;
  if (A.E_cap > 0 && (!A.edge_event || !A.ei_jj)) return GGNN_EINVAL;
  const int64_t nblk = (A.n_grain + A.E_cap + 255) / 256;
  if (nblk >= INT32_MAX) return GGNN_EINVAL;
  const size_t n_flags = A.range_word ? 3 : 2, n_counts = is_union ? 2 * (size_t)A.n_traj : 0;
  const bool one = is_union && A.counts == A.flags + n_flags;   // one buffer, the totals first: one memset
  if (hipMemsetAsync(A.flags, 0, (n_flags + (one ? n_counts : 0)) * sizeof(int32_t), stream) != hipSuccess) return GGNN_ELAUNCH;
  if (is_union && !one && hipMemsetAsync(A.counts, 0, n_counts * sizeof(int32_t), stream) != hipSuccess) return GGNN_ELAUNCH;
  hipLaunchKernelGGL(is_union ? detect_events_kernel<true> : detect_events_kernel<false>, dim3((unsigned)nblk), dim3(256), 0,
                     stream, A);
  return launch_status();
}

}  // namespace ggnn

extern "C" int ggnn_step_update(float* x_joint, int64_t n_joint, int64_t ldx_joint, float* x_grain,
                                int64_t n_grain, int64_t ldx_grain, int f_grain,
                                const float* y_joint, const float* y_grain, float dz, float zmax,
                                int32_t* flags, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!x_joint || !x_grain || !y_joint || !y_grain || !flags) return GGNN_EINVAL;
  if (n_joint <= 0 || n_grain <= 0 || ldx_joint < 8 || f_grain < 6 || ldx_grain < f_grain)
    return GGNN_EINVAL;
  const int64_t nblk = (n_joint + n_grain + 255) / 256;
  if (nblk >= INT32_MAX) return GGNN_EINVAL;
  hipLaunchKernelGGL(step_update_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream,
                     x_joint, n_joint, ldx_joint, x_grain, n_grain, ldx_grain, f_grain, y_joint,
                     y_grain, dz, zmax, flags);
  return launch_status();
}

extern "C" int ggnn_grain_centres(const int32_t* rowptr, const int32_t* col, const float* x_joint, int64_t n_joint,
                                  int64_t ldx_joint, const float* domain_offset, float domain_factor, float* x_grain,
                                  int64_t n_grain, int64_t ldx_grain, float* centres_before, int boundary,
                                  ggnn_stream_t stream) {
  using namespace ggnn;
  if (boundary != GGNN_BC_PERIODIC && boundary != GGNN_BC_NOFLUX) return GGNN_EINVAL;
  if (!rowptr || !col || !x_joint || !x_grain) return GGNN_EINVAL;
  if (n_joint <= 0 || n_grain <= 0 || ldx_joint < 2 || ldx_grain < 2) return GGNN_EINVAL;
  if (!(domain_factor >= 1.0f)) return GGNN_EINVAL;
  const int64_t nblk = (n_grain + 255) / 256;
  if (nblk >= INT32_MAX) return GGNN_EINVAL;
  const auto kernel = boundary == GGNN_BC_PERIODIC ? grain_centres_kernel<true> : grain_centres_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, rowptr, col, x_joint, ldx_joint,
                     domain_offset, domain_factor, x_grain, ldx_grain, n_grain, n_joint, centres_before);
  return launch_status();
}

extern "C" int ggnn_noflux_boundary_traj(const int32_t* rowptr_jg, const int32_t* col_jg, float* x_joint, int64_t n_joint,
                                         int64_t ldx_joint, const float* domain_offset, float domain_factor, float max_y,
                                         float* x_grain, int64_t ldx_grain, int f_grain, float* joints_before,
                                         const int64_t* traj_grain_off, const int64_t* traj_joint_off, int64_t n_traj,
                                         ggnn_stream_t stream) {
  if (!ggnn::seg_union_ok(traj_grain_off, n_traj, false) || !traj_joint_off) return GGNN_EINVAL;
  return ggnn::launch_noflux_boundary(rowptr_jg, col_jg, x_joint, n_joint, ldx_joint, domain_offset, domain_factor, max_y, x_grain,
                                      ldx_grain, f_grain, joints_before, traj_grain_off, traj_joint_off, (int)n_traj,
                                      (hipStream_t)stream);
}

// (one rollout = the one-trajectory case of the kernel: every junction, boundary grain 0)
extern "C" int ggnn_noflux_boundary(const int32_t* rowptr_jg, const int32_t* col_jg, float* x_joint, int64_t n_joint,
                                    int64_t ldx_joint, const float* domain_offset, float domain_factor, float max_y,
                                    float* x_grain, int64_t ldx_grain, int f_grain, float* joints_before,
                                    ggnn_stream_t stream) {
  return ggnn::launch_noflux_boundary(rowptr_jg, col_jg, x_joint, n_joint, ldx_joint, domain_offset, domain_factor, max_y, x_grain,
                                      ldx_grain, f_grain, joints_before, nullptr, nullptr, 1, (hipStream_t)stream);
}

extern "C" int ggnn_process_schedule(float* x_joint, int64_t n_joint, int64_t ldx_joint, const float* table, int64_t n_rows,
                                     int64_t n_traj, const int64_t* traj_joint_off, const int32_t* step_in, int32_t* step_out,
                                     int32_t* sync_word, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!x_joint || !table || !step_in || !step_out || !sync_word) return GGNN_EINVAL;
  if (n_joint <= 0 || ldx_joint < 5 || n_rows < 1 || !seg_union_ok(traj_joint_off, n_traj, true)) return GGNN_EINVAL;
  const int64_t nblk = (n_joint + 255) / 256;
  if (nblk >= INT32_MAX) return GGNN_EINVAL;
  hipLaunchKernelGGL(process_schedule_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, x_joint, n_joint,
                     ldx_joint, table, n_rows, (int)n_traj, traj_joint_off, step_in, step_out, sync_word);
  return launch_status();
}

extern "C" int ggnn_detect_events(const float* grain_area, const int32_t* live_grain, int64_t n_grain,
                                  float area_threshold, const float* edge_event, const int64_t* edge_index_jj,
                                  int64_t E, const int64_t* E_dev, float logit_threshold, int32_t* flags,
                                  int32_t* range_word, int64_t skip_grain, ggnn_stream_t stream) {
  const ggnn::detect_kargs A = {grain_area, live_grain, edge_event, edge_index_jj, E_dev, flags, range_word, n_grain, E,
                                area_threshold, logit_threshold, skip_grain, nullptr, nullptr, nullptr, nullptr, 1};
  return ggnn::launch_detect_events(A, false, (hipStream_t)stream);
}

extern "C" int ggnn_detect_events_traj(const float* grain_area, const int32_t* live_grain, int64_t n_grain,
                                       float area_threshold, const float* edge_event, const int64_t* edge_index_jj,
                                       int64_t E, const int64_t* E_dev, float logit_threshold,
                                       const int64_t* traj_grain_off, const int64_t* traj_joint_off, int64_t n_traj,
                                       const int32_t* ended, int64_t skip_local_grain, int32_t* counts, int32_t* flags,
                                       int32_t* range_word, ggnn_stream_t stream) {
  if (!counts || !ggnn::seg_union_ok(traj_grain_off, n_traj, false) || !traj_joint_off) return GGNN_EINVAL;
  if (skip_local_grain != -1) return GGNN_EINVAL;   // (no-flux unions keep their boundary grains out through live_grain)
  const ggnn::detect_kargs A = {grain_area, live_grain, edge_event, edge_index_jj, E_dev, flags, range_word, n_grain, E,
                                area_threshold, logit_threshold, -1, traj_grain_off, traj_joint_off, ended, counts, (int)n_traj};
  return ggnn::launch_detect_events(A, true, (hipStream_t)stream);
}

extern "C" int ggnn_step_refresh(float* x_joint, int64_t n_joint, int64_t ldx_joint,
                                 float* x_grain, int64_t n_grain, int64_t ldx_grain, float zmax,
                                 const int32_t* flags, const ggnn_refresh_edge* edges,
                                 int n_edge_types, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!x_joint || !x_grain || !flags || n_joint <= 0 || n_grain <= 0) return GGNN_EINVAL;
  if (ldx_joint < 3 || ldx_grain < 3) return GGNN_EINVAL;
  if (n_edge_types < 0 || n_edge_types > 3 || (n_edge_types > 0 && !edges)) return GGNN_EINVAL;
  RefreshArgs R;
  R.n_et = n_edge_types;
  R.e_off[0] = 0;
  for (int k = 0; k < 3; ++k) {
    if (k < n_edge_types) {
      const ggnn_refresh_edge& T = edges[k];
      if (T.E < 0 || T.ldx_src < 2 || T.ldx_dst < 2 || T.n_src <= 0 || T.n_dst <= 0) return GGNN_EINVAL;
      if (T.E > 0 && (!T.edge_index || !T.x_src || !T.x_dst || !T.edge_attr)) return GGNN_EINVAL;
      R.et[k] = T;
      R.e_off[k + 1] = R.e_off[k] + T.E;
    } else {
      R.et[k] = ggnn_refresh_edge{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0};
      R.e_off[k + 1] = R.e_off[k];
    }
  }
  const int64_t total = n_joint + n_grain + R.e_off[n_edge_types];
  const int64_t nblk = (total + 255) / 256;
  if (nblk >= INT32_MAX) return GGNN_EINVAL;
  hipLaunchKernelGGL(step_refresh_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream,
                     x_joint, n_joint, ldx_joint, x_grain, n_grain, ldx_grain, zmax, flags, R);
  return launch_status();
}
