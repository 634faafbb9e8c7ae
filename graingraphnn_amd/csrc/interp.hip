// In-between layers of a rollout (test.py:494-528, --interp_frames): polygon records of positions blended from two recorded
// layers, with the topology of the nearer one.
//   ggnn_interp_polygons = up to GGNN_INTERP_MAX_JOBS jobs (layer L, coefficient c), the job a grid dimension, in two or
//                          three launches: blend -> (no-flux) snap -> rows.  The rule is include/ggnn.h's.
// The positions are finished per junction in a workspace before any row reads them: a junction is held by three grains, and
// all three must see it where move_to_boundary left it.  The blend launch writes every junction (no-flux: clamped to the
// box); the snap launch walks the boundary grains' rows of layer T's table, forms the unclamped blend of those junctions
// again with the same device function -- the same bits -- and overwrites the one coordinate that goes to a wall.  It reads
// recorded layers only and writes a value that depends on nothing else, so a junction listed twice is written twice the
// same.  The rows are polygon_rows.h's, the code ggnn_grain_polygons runs, on the workspace with domain_factor 1.
// Every product and sum of the blend is rounded on its own (fp contract(off) round them: nothing meets in an fma), so a
// numpy restatement gives the same bits (tests/interpcheck.py), and c = 1 / c = 0 return a layer's own positions.
#include "polygon_rows.h"

namespace ggnn {

struct InterpJobs {   // a kernel argument, as the rasteriser's layers are
  int32_t layer[GGNN_INTERP_MAX_JOBS];
  float c[GGNN_INTERP_MAX_JOBS], rest[GGNN_INTERP_MAX_JOBS];   // fl(c), fl(1 - c)
  uint8_t upper[GGNN_INTERP_MAX_JOBS];                         // the topology is layer L's (c > 0.5), not layer L - 1's
};

struct InterpJob {
  int64_t L, T;   // clamped: rows L - 1, L and T exist
  float c, rest;
};

__device__ __forceinline__ InterpJob interp_job(const ggnn_interp_args& A, const InterpJobs& J, int job) {
  const int64_t L = min(max((int64_t)J.layer[job], (int64_t)1), max(A.capacity, (int64_t)1));
  return {L, J.upper[job] ? L : L - 1, J.c[job], J.rest[job]};
}

// Junction j of a job before the walls: seam, blend, wrap.
template <bool PERIODIC>
__device__ __forceinline__ void interp_blend(const ggnn_interp_args& A, const InterpJob& B, int64_t j, float v[2]) {
  const float* hi = A.joint_xy + 2 * (B.L * A.n_joint + j);
  const float* lo = A.joint_xy + 2 * ((B.L - 1) * A.n_joint + j);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    float xl = hi[k], xp = lo[k];
    const float t = B.T == B.L ? xl : xp;   // layer T's own coordinate
    if (PERIODIC) {
      if (B.T == B.L) xp = min_image(xp, xl);
      else xl = min_image(xl, xp);
    }
    float w;
    {   // (the products and the sum must not meet in an fma; __fmul_rn / __fadd_rn are plain operators the compiler contracts)
#pragma clang fp contract(off)
      const float a = B.c * xl, b = B.rest * xp;
      w = a + b;
    }
    // (a recorded coordinate may itself lie outside [0, 1) -- the junctions are never wrapped -- and is then left where it
    //  is: c = 1 and c = 0 return the layers' own positions)
    if (PERIODIC && !(w >= 0.0f && w < 1.0f) && t >= 0.0f && t < 1.0f) w = __fsub_rn(w, floorf(w));
    v[k] = w;
  }
}

template <bool PERIODIC>
__global__ __launch_bounds__(POLY_BLOCK) void interp_blend_kernel(const ggnn_interp_args A, const InterpJobs J) {
  const int job = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * POLY_BLOCK + threadIdx.x;
  if (j >= A.n_joint) return;
  const InterpJob B = interp_job(A, J, job);
  float v[2];
  interp_blend<PERIODIC>(A, B, j, v);
  if (!PERIODIC) {   // test.py:505-508
    const float top[2] = {1.0f, A.max_y};
#pragma unroll
    for (int k = 0; k < 2; ++k) v[k] = v[k] < 0.0f ? 0.0f : (v[k] > top[k] ? top[k] : v[k]);
  }
  float* out = A.work + 2 * ((int64_t)job * A.n_joint + j);
  out[0] = v[0];
  out[1] = v[1];
}

// move_to_boundary (test.py:58-70) for the junctions of a trajectory's boundary grain: block (t, job).
__global__ __launch_bounds__(POLY_BLOCK) void interp_snap_kernel(const ggnn_interp_args A, const InterpJobs J) {
  const int job = blockIdx.y;
  const int64_t t = blockIdx.x;
  int64_t g = 0;
  if (A.traj_grain_off != nullptr) {
    g = A.traj_grain_off[t];
    if (g < 0 || g >= A.traj_grain_off[t + 1]) return;   // a trajectory without grains
  }
  if (g >= A.n_grain) return;
  const InterpJob B = interp_job(A, J, job);
  const int32_t* rowptr = A.rowptr + B.T * (A.n_grain + 1);
  const int32_t* col = A.col + B.T * A.E_cap;
  const int64_t p0 = min((int64_t)max(rowptr[g], 0), A.E_cap);
  const int64_t p1 = min((int64_t)max((int64_t)rowptr[g + 1], p0), A.E_cap);
  for (int64_t e = p0 + threadIdx.x; e < p1; e += POLY_BLOCK) {
    const int64_t j = min((int64_t)max(col[e], 0), A.n_joint - 1);
    float v[2];
    interp_blend<false>(A, B, j, v);
    const float d[4] = {v[0], __fsub_rn(1.0f, v[0]), v[1], __fsub_rn(A.max_y, v[1])};
    int k = 0;
    float m = d[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {   // torch.argmin keeps the first of equal minima
      const bool lower = d[i] < m;
      m = lower ? d[i] : m;
      k = lower ? i : k;
    }
    A.work[2 * ((int64_t)job * A.n_joint + j) + (k >> 1)] = k == 0 ? 0.0f : (k == 1 ? 1.0f : (k == 2 ? 0.0f : A.max_y));
  }
}

template <bool PERIODIC>
__global__ __launch_bounds__(POLY_BLOCK) void interp_rows_kernel(const ggnn_interp_args A, const InterpJobs J) {
  const int64_t job = blockIdx.y;
  const InterpJob B = interp_job(A, J, (int)job);
  const PolyIn I = {A.col + B.T * A.E_cap, A.work + 2 * job * A.n_joint, nullptr, 2, A.n_joint, 1.0f};
  const PolyOut O = {A.joint_sorted + job * A.E_cap, A.xy_sorted + 2 * job * A.E_cap, A.centre + 2 * job * A.n_grain,
                     A.area + job * A.n_grain};
  poly_block_rows<PERIODIC>(I, O, A.rowptr + B.T * (A.n_grain + 1), A.rowptr_out + job * (A.n_grain + 1), A.n_grain, A.E_cap,
                            A.traj_grain_off, A.n_traj);
}

}  // namespace ggnn

extern "C" int ggnn_interp_polygons(const ggnn_interp_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_interp_args& A = *args;
  if (A.boundary != GGNN_BC_PERIODIC && A.boundary != GGNN_BC_NOFLUX) return GGNN_EINVAL;
  if (!A.rowptr || !A.col || !A.joint_xy || !A.job_layer || !A.job_coeff || !A.work) return GGNN_EINVAL;
  if (!A.rowptr_out || !A.joint_sorted || !A.xy_sorted || !A.centre || !A.area) return GGNN_EINVAL;
  if (A.n_joint <= 0 || A.n_grain <= 0 || A.E_cap < 0 || A.E_cap >= INT32_MAX) return GGNN_EINVAL;
  if (A.capacity < 0 || A.capacity >= INT32_MAX || A.layers < 1 || A.layers > A.capacity) return GGNN_EINVAL;
  if (A.n_jobs < 1 || A.n_jobs > GGNN_INTERP_MAX_JOBS) return GGNN_EINVAL;
  if (A.boundary == GGNN_BC_NOFLUX && !(A.max_y > 0.0f)) return GGNN_EINVAL;
  if (!seg_union_ok(A.traj_grain_off, A.n_traj, true)) return GGNN_EINVAL;
  InterpJobs J = {};
  for (int64_t i = 0; i < A.n_jobs; ++i) {
    const double c = A.job_coeff[i];
    if (!(c >= 0.0 && c <= 1.0) || A.job_layer[i] < 1 || A.job_layer[i] > A.layers) return GGNN_EINVAL;
    J.layer[i] = A.job_layer[i];
    J.c[i] = (float)c;
    J.rest[i] = (float)(1.0 - c);   // formed in double, rounded once, as the reference's Python does
    J.upper[i] = c > 0.5 ? 1 : 0;
  }
  const int64_t jblk = (A.n_joint + POLY_BLOCK - 1) / POLY_BLOCK, gblk = (A.n_grain + POLY_GRAINS - 1) / POLY_GRAINS;
  if (jblk >= INT32_MAX || gblk >= INT32_MAX) return GGNN_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  const bool periodic = A.boundary == GGNN_BC_PERIODIC;
  const unsigned jobs = (unsigned)A.n_jobs;
  hipLaunchKernelGGL(periodic ? interp_blend_kernel<true> : interp_blend_kernel<false>, dim3((unsigned)jblk, jobs),
                     dim3(POLY_BLOCK), 0, st, A, J);
  if (!periodic) hipLaunchKernelGGL(interp_snap_kernel, dim3((unsigned)A.n_traj, jobs), dim3(POLY_BLOCK), 0, st, A, J);
  hipLaunchKernelGGL(periodic ? interp_rows_kernel<true> : interp_rows_kernel<false>, dim3((unsigned)gblk, jobs),
                     dim3(POLY_BLOCK), 0, st, A, J);
  return launch_status();
}
