// The grains' junction polygons of a rollout layer, recorded on the device next to the step: what graph.update()
// (graph_datastruct.py:654-721) leaves in `regions`, `region_coors` and `region_center`.
//   ggnn_grain_polygons = one layer, one launch: per grain the junctions of its row of the joint->grain table, unwrapped as
//                         grain_centres_kernel (step.hip) unwraps them, ordered counter-clockwise round their mean by the
//                         key of counterclock() (:100-116), with the mean and the shoelace area of the ordered polygon
//   ggnn_polygon_inputs = the table's columns and the junctions' global positions of that layer, kept beside its record
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
// The row code itself lives in polygon_rows.h, which ggnn_interp_polygons (interp.hip) shares.
#include "polygon_rows.h"

namespace ggnn {

template <bool PERIODIC>
__global__ __launch_bounds__(POLY_BLOCK) void grain_polygons_kernel(const ggnn_polygon_args A) {
  // the layer this launch writes: read by every block before the last one to finish advances the counter
  const int64_t k = A.layer_in ? (int64_t)*A.layer_in + 1 : 0;
  const bool room = k >= 0 && k <= A.capacity;
  if (room) {   // (block-uniform)
    const PolyIn I = {A.col, A.x_joint, A.domain_offset, A.ldx_joint, A.n_joint, A.domain_factor};
    const PolyOut O = {A.joint_sorted + k * A.E_cap, A.xy_sorted + 2 * k * A.E_cap, A.centre + 2 * k * A.n_grain,
                       A.area + k * A.n_grain};
    poly_block_rows<PERIODIC>(I, O, A.rowptr, A.rowptr_out + k * (A.n_grain + 1), A.n_grain, A.E_cap, A.traj_grain_off,
                              A.n_traj);
  }
  // the last block to get here has seen every other block read the counter
  if (A.layer_out != nullptr) {
    __syncthreads();
    if (threadIdx.x == 0) {
      __threadfence();
      if (atomicAdd(A.sync_word, 1) == (int32_t)gridDim.x - 1) {
        *A.sync_word = 0;
        *A.layer_out = (int32_t)min(k, (int64_t)INT32_MAX);
        if (!room) atomicOr(A.flags, GGNN_FLAG_POLYGON_OVERFLOW);
      }
    }
  }
}

// What the layer's polygon launch reads, kept for ggnn_interp_polygons: thread i copies table entry i and writes junction i
// in the global frame, to the row the polygon launch behind this one will write (it advances the word, this launch does not).
__global__ __launch_bounds__(POLY_BLOCK) void polygon_inputs_kernel(const ggnn_polygon_inputs_args A) {
  const int64_t k = A.layer_in ? (int64_t)*A.layer_in + 1 : 0;
  if (k < 0 || k > A.capacity) return;
  const int64_t i = (int64_t)blockIdx.x * POLY_BLOCK + threadIdx.x;
  if (i < A.E_cap) A.col_out[k * A.E_cap + i] = A.col[i];
  if (i < A.n_joint) {
    const PolyIn I = {A.col, A.x_joint, A.domain_offset, A.ldx_joint, A.n_joint, A.domain_factor};
    float x, y;
    I.global_xy(i, x, y);
    float* out = A.joint_xy + 2 * (k * A.n_joint + i);
    out[0] = x;
    out[1] = y;
  }
}

}  // namespace ggnn

extern "C" int ggnn_polygon_inputs(const ggnn_polygon_inputs_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_polygon_inputs_args& A = *args;
  if (!A.col || !A.x_joint || !A.col_out || !A.joint_xy) return GGNN_EINVAL;
  if (A.n_joint <= 0 || A.ldx_joint < 2 || A.E_cap < 0 || A.E_cap >= INT32_MAX) return GGNN_EINVAL;
  if (!(A.domain_factor >= 1.0f) || A.capacity < 0 || A.capacity >= INT32_MAX) return GGNN_EINVAL;
  const int64_t nblk = (std::max(A.n_joint, A.E_cap) + POLY_BLOCK - 1) / POLY_BLOCK;
  if (nblk >= INT32_MAX) return GGNN_EINVAL;
  hipLaunchKernelGGL(polygon_inputs_kernel, dim3((unsigned)nblk), dim3(POLY_BLOCK), 0, (hipStream_t)stream, A);
  return launch_status();
}

extern "C" int ggnn_grain_polygons(const ggnn_polygon_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_polygon_args& A = *args;
  if (A.boundary != GGNN_BC_PERIODIC && A.boundary != GGNN_BC_NOFLUX) return GGNN_EINVAL;
  if (!A.rowptr || !A.col || !A.x_joint || !A.rowptr_out || !A.joint_sorted || !A.xy_sorted || !A.centre || !A.area)
    return GGNN_EINVAL;
  if (A.n_joint <= 0 || A.n_grain <= 0 || A.ldx_joint < 2 || A.E_cap < 0 || A.E_cap >= INT32_MAX) return GGNN_EINVAL;
  if (!(A.domain_factor >= 1.0f) || A.capacity < 0 || A.capacity >= INT32_MAX) return GGNN_EINVAL;
  if (!seg_union_ok(A.traj_grain_off, A.n_traj, true)) return GGNN_EINVAL;
  if (A.layer_out && (!A.sync_word || !A.flags)) return GGNN_EINVAL;
  const int64_t nblk = (A.n_grain + POLY_GRAINS - 1) / POLY_GRAINS;
  if (nblk >= INT32_MAX) return GGNN_EINVAL;
  const auto kernel = A.boundary == GGNN_BC_PERIODIC ? grain_polygons_kernel<true> : grain_polygons_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(POLY_BLOCK), 0, (hipStream_t)stream, A);
  return launch_status();
}
