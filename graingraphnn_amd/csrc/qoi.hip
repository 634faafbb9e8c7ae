// Quantities of interest of a rollout, accumulated on the device next to the step (graph_trajectory.py:1042-1051 "qoi",
// :221-242 volume('graph'), :244-256 qoi):
//   ggnn_qoi_accumulate = one layer: the normalised live-grain areas a_k, the scaled excess volumes e_k, the trapezoid
//                         integral T_k of the areas over the layers, optionally row k of the history of volume_k
//   ggnn_qoi_finalize   = volume, equivalent diameter, and per trajectory d_mu, d_std and histogram counts
// Every grain's arithmetic and every sum runs in fp64 and is rounded to fp32 where it is stored; the sums are trees of a
// FIXED shape over the trajectory's grains, anchored at its first grain: no floating-point atomics, the same bits for any
// grid and at any position of the trajectory in a union.
#include "common.h"

namespace ggnn {

constexpr int QOI_BLOCK = 256;

template <int CTRL>
__device__ __forceinline__ double dpp_add_d(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, 0xF, 0xF, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, 0xF, 0xF, true);
  return v + __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// Sum over the block's 256 threads, the same value in every thread: four DPP steps inside each row of 16 lanes (as
// row_sum, on the two halves of a double), then the 16 row sums in index order.  Every thread of the block must call it.
__device__ __forceinline__ double block_sum_d(double v, double* s_red) {
  v = dpp_add_d<0xB1>(v);    // quad_perm [1,0,3,2]
  v = dpp_add_d<0x4E>(v);    // quad_perm [2,3,0,1]
  v = dpp_add_d<0x141>(v);   // row_half_mirror
  v = dpp_add_d<0x140>(v);   // row_mirror
  __syncthreads();           // (s_red of the call before has been read)
  if ((threadIdx.x & 15) == 0) s_red[threadIdx.x >> 4] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < QOI_BLOCK / 16; ++i) t += s_red[i];
  return t;
}

// The trajectory and the 256-grain chunk of it that block `b` works on: chunks are counted from each trajectory's first
// grain, trajectory after trajectory.  Returns false for a block behind the last chunk (the launch is sized by an upper
// bound).  Offsets outside [0, n_grain] are clamped: nothing is ever addressed outside the arrays.
// (A walk over the trajectories' chunk counts, not segments.h's "which segment holds node v".)
__device__ __forceinline__ bool qoi_block_range(const int64_t* __restrict__ off, int64_t n_traj, int64_t n_grain, int64_t b,
                                                int64_t& traj, int64_t& lo, int64_t& n, int64_t& chunk) {
  for (int64_t t = 0; t < n_traj; ++t) {
    const int64_t a = min(max(off[t], (int64_t)0), n_grain), z = min(max(off[t + 1], a), n_grain);
    const int64_t nb = (z - a + QOI_BLOCK - 1) / QOI_BLOCK;
    if (b < nb) {
      traj = t, lo = a, n = z - a, chunk = b;
      return true;
    }
    b -= nb;
  }
  return false;
}

__global__ __launch_bounds__(QOI_BLOCK) void qoi_accumulate_kernel(const ggnn_qoi_args A) {
  __shared__ double s_red[QOI_BLOCK / 16];
  const int tid = threadIdx.x;
  // the layer this launch writes: read by every block before the last one to finish advances the counter (which may be
  // the same word: a captured graph replays with the counter where the replay before left it)
  const int32_t k = A.init ? 0 : *A.layer_in + 1;
  int64_t traj = 0, lo = 0, n = 0, chunk = 0;
  if (qoi_block_range(A.traj_offsets, A.n_traj, A.n_grain, blockIdx.x, traj, lo, n, chunk)) {
    // A_k of the whole trajectory, by every block of it: thread t takes grains t, t + 256, ... of the trajectory
    double sum = 0.0, cnt = 0.0;
    for (int64_t i = tid; i < n; i += QOI_BLOCK) {
      const int64_t g = lo + i;
      if (A.live_grain == nullptr || A.live_grain[g] > 0) {
        sum += (double)A.x_grain[g * A.ldx_grain + 3];
        cnt += 1.0;
      }
    }
    sum = block_sum_d(sum, s_red);
    cnt = block_sum_d(cnt, s_red);
    const double area_sum = sum / (A.domain_factor * A.domain_factor);
    if (chunk == 0 && tid == 0 && A.area_sum != nullptr) A.area_sum[traj] = (float)area_sum;
    const int64_t i = chunk * QOI_BLOCK + tid;
    if (i < n) {
      const int64_t g = lo + i;
      const float* x = A.x_grain + g * A.ldx_grain;
      const bool live = A.live_grain == nullptr || A.live_grain[g] > 0;
      const double s2 = A.s * A.s;
      float a = live && cnt > 0.0 ? (float)((double)x[3] * s2 / area_sum) : 0.0f;
      const float e = live ? (float)((double)x[4] / 20.0 * (s2 * A.s)) : 0.0f;   // targets_scaling['grain'] = 20
      float T, vol;
      if (A.init) {
        if (A.area0 != nullptr) a = A.area0[g];
        const double v0 = 4.0 / 3.0 / sqrt(M_PI) * ((double)a * sqrt((double)a));
        A.V0[g] = (float)v0;
        T = 0.0f;
        vol = (float)v0;   // (volume_traj[0] carries no excess volume: graph_trajectory.py:230)
      } else {
        T = (float)((double)A.T_in[g] + 0.5 * A.delta_h * ((double)A.a_prev[g] + (double)a));
        vol = (float)((double)A.V0[g] + (double)T + (double)e);
      }
      A.a_cur[g] = a;
      A.T_out[g] = T;
      A.e_cur[g] = e;
      if (A.history != nullptr && k <= A.capacity) A.history[(int64_t)k * A.n_grain + g] = vol;
    }
  }
  // the last block to get here has seen every other block read the counter
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    if (atomicAdd(A.sync_word, 1) == (int32_t)gridDim.x - 1) {
      *A.sync_word = 0;
      *A.layer_out = k;
      if (A.history != nullptr && k > A.capacity) atomicOr(A.flags, GGNN_FLAG_QOI_OVERFLOW);
    }
  }
}

constexpr int QOI_MAX_BINS = 1024;

__global__ __launch_bounds__(QOI_BLOCK) void qoi_finalize_kernel(
    const float* __restrict__ V0, const float* __restrict__ T, const float* __restrict__ e, int64_t n_grain,
    const int64_t* __restrict__ off, double mesh_size, const float* __restrict__ edges, int n_edges,
    float* __restrict__ volume, float* __restrict__ size, float* __restrict__ d_mu, float* __restrict__ d_std,
    int32_t* __restrict__ hist) {
  __shared__ double s_red[QOI_BLOCK / 16];
  __shared__ int32_t s_hist[QOI_MAX_BINS];
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  const int64_t lo = min(max(off[t], (int64_t)0), n_grain), hi = min(max(off[t + 1], lo), n_grain);
  const int n_bins = n_edges - 1;
  for (int b = tid; b < n_bins; b += QOI_BLOCK) s_hist[b] = 0;
  double sum = 0.0;
  for (int64_t g = lo + tid; g < hi; g += QOI_BLOCK) {
    const double v = (double)V0[g] + (double)T[g] + (double)e[g];
    const float d = (float)(cbrt(6.0 * v / M_PI) * mesh_size);
    volume[g] = (float)v;
    size[g] = d;
    sum += (double)d;
  }
  const double count = (double)(hi - lo);
  const double mean = block_sum_d(sum, s_red) / count;   // (an empty trajectory: NaN, as np.mean of nothing)
  double sq = 0.0;
  for (int64_t g = lo + tid; g < hi; g += QOI_BLOCK) {
    const float d = size[g];   // (written by this thread)
    sq += ((double)d - mean) * ((double)d - mean);
    if (n_bins > 0 && d >= edges[0] && d <= edges[n_bins]) {   // np.histogram: [e_i, e_i+1), the last bin closed
      int a = 0, z = n_bins;                                   // the last edge <= d
      while (z - a > 1) {
        const int m = (a + z) >> 1;
        if (d >= edges[m]) a = m; else z = m;
      }
      atomicAdd(&s_hist[a], 1);
    }
  }
  const double var = block_sum_d(sq, s_red) / count;
  if (tid == 0) {
    d_mu[t] = (float)mean;
    d_std[t] = (float)sqrt(var);
  }
  __syncthreads();
  for (int b = tid; b < n_bins; b += QOI_BLOCK) hist[t * n_bins + b] = s_hist[b];
}

}  // namespace ggnn

extern "C" int ggnn_qoi_accumulate(const ggnn_qoi_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_qoi_args& A = *args;
  if (!A.x_grain || !A.traj_offsets || !A.a_cur || !A.T_out || !A.e_cur || !A.V0 || !A.layer_out || !A.sync_word || !A.flags)
    return GGNN_EINVAL;
  if (!A.init && (!A.a_prev || !A.T_in || !A.layer_in)) return GGNN_EINVAL;
  if (A.n_grain <= 0 || A.n_traj <= 0 || A.ldx_grain < 5 || A.capacity < 0 || A.capacity >= INT32_MAX) return GGNN_EINVAL;
  if (!(A.domain_factor >= 1.0) || !(A.s > 0.0) || !(A.delta_h == A.delta_h)) return GGNN_EINVAL;
  // an upper bound of the chunks: sum ceil(n_t / 256) <= n_grain / 256 + n_traj
  const int64_t nblk = (A.n_grain + QOI_BLOCK - 1) / QOI_BLOCK + A.n_traj;
  if (nblk >= INT32_MAX) return GGNN_EINVAL;
  hipLaunchKernelGGL(qoi_accumulate_kernel, dim3((unsigned)nblk), dim3(QOI_BLOCK), 0, (hipStream_t)stream, A);
  return launch_status();
}

extern "C" int ggnn_qoi_finalize(const float* V0, const float* T, const float* e, int64_t n_grain,
                                 const int64_t* traj_offsets, int64_t n_traj, double mesh_size, const float* bin_edges,
                                 int n_edges, float* volume, float* size, float* d_mu, float* d_std, int32_t* hist,
                                 ggnn_stream_t stream) {
  using namespace ggnn;
  if (!V0 || !T || !e || !traj_offsets || !volume || !size || !d_mu || !d_std) return GGNN_EINVAL;
  if (n_grain <= 0 || n_traj <= 0 || n_traj >= INT32_MAX || !(mesh_size > 0.0)) return GGNN_EINVAL;
  if (n_edges < 0 || n_edges == 1 || n_edges > QOI_MAX_BINS + 1 || (n_edges > 0 && (!bin_edges || !hist))) return GGNN_EINVAL;
  hipLaunchKernelGGL(qoi_finalize_kernel, dim3((unsigned)n_traj), dim3(QOI_BLOCK), 0, (hipStream_t)stream, V0, T, e, n_grain,
                     traj_offsets, mesh_size, bin_edges, n_edges, volume, size, d_mu, d_std, hist);
  return launch_status();
}
