// Validation metrics (metrics.py:23-72 feature_metric.record, :124-217 the precision / recall counts): one validation batch
// = ONE launch that adds into a device-resident accumulator (include/ggnn.h, ggnn_metric_record).  The reference reads five
// scalars back per batch and counts the true / false positives element by element through the interpreter; here nothing
// leaves the device before the epoch's summary.  The workload is tiny (<= 60 000 elements per term): the kernel is bound by
// its launch and is not tuned beyond being one.
//
// The structure is masked_mse_kernel's (train_misc.hip): GGNN_METRIC_BLOCKS workgroups, each over a fixed share of the
// elements in a grid-stride loop; wave64 reductions (shuffles for the fp64 sums, ballot + popcount for the counts); the
// workgroups' partial results go through the workspace and the last workgroup to arrive at an integer ticket adds them in
// index order INTO the accumulator.  No floating-point atomics: the fp64 slots have the same bits on every run.
#include "common.h"

namespace ggnn {

constexpr int MT_THREADS = 256, MT_WAVES = MT_THREADS / 64;
constexpr int MT_F64 = 2 * GGNN_METRIC_MAX_TERMS;   // err[4] | norm[4] per workgroup
constexpr int MT_CNT = 3 * GGNN_METRIC_MAX_THR;     // TP[16] | FP[16] | FN[16] per workgroup
constexpr int MT_ROW = MT_F64 + MT_CNT;             // 8-byte words of a workgroup's row in the workspace
static_assert(GGNN_METRIC_WS_WORDS == GGNN_METRIC_BLOCKS * MT_ROW + 1, "workspace layout");
static_assert(GGNN_METRIC_F64_SLOTS == MT_F64 + 1 && GGNN_METRIC_I64_SLOTS == MT_CNT + 1, "accumulator layout");

__global__ __launch_bounds__(MT_THREADS) void metric_record_kernel(const ggnn_metric_args A) {
  __shared__ double red[MT_WAVES][MT_F64];
  __shared__ unsigned cnt[MT_WAVES][MT_CNT];
  __shared__ int is_last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t gtid = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x, gstride = (int64_t)GGNN_METRIC_BLOCKS * MT_THREADS;

  // ---- squared-error terms: sum m (y - p)^2 and, in the first epoch, sum m y^2; fp64 from the fp32 inputs ----
  double s[MT_F64];
#pragma unroll
  for (int k = 0; k < MT_F64; ++k) s[k] = 0.0;
#pragma unroll
  for (int k = 0; k < GGNN_METRIC_MAX_TERMS; ++k) {
    if (k >= A.n_terms) continue;
    const float* __restrict__ p = A.pred[k] + A.col[k];
    const float* __restrict__ y = A.target[k] + A.col[k];
    const float* __restrict__ m = A.mask[k];
    const int64_t n = A.n_rows[k], ld = A.ld[k], ldm = A.ld_mask[k];
    double err = 0.0, norm = 0.0;
    for (int64_t r = gtid; r < n; r += gstride) {
      const float w = m[r * ldm];
      if (w != 0.f) {   // (a masked row adds exactly 0, whatever its prediction holds)
        const double yv = (double)y[r * ld], d = yv - (double)p[r * ld];
        err += (double)w * (d * d);
        norm += (double)w * (yv * yv);
      }
    }
    s[k] = err;
    s[GGNN_METRIC_MAX_TERMS + k] = A.with_norm ? norm : 0.0;
  }
#pragma unroll
  for (int k = 0; k < MT_F64; ++k) {
    double v = s[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) red[wave][k] = v;
  }

  // ---- threshold term: per threshold TP / FP / FN, a ballot and a popcount per wave and step (wave-uniform counters) ----
  unsigned tp[GGNN_METRIC_MAX_THR], fp[GGNN_METRIC_MAX_THR], fn[GGNN_METRIC_MAX_THR];
#pragma unroll
  for (int j = 0; j < GGNN_METRIC_MAX_THR; ++j) tp[j] = fp[j] = fn[j] = 0u;
  const bool classifier = A.mode == GGNN_METRIC_CLASSIFIER;
  // (the loop runs on the wave's first element so that all 64 lanes take every step together)
  for (int64_t base = gtid - lane; base < A.n; base += gstride) {
    const int64_t i = base + lane;
    bool counted = false, one = false, zero = false;
    float sc = 0.f;
    if (i < A.n) {
      const int64_t lab = A.label[i];
      one = lab == 1, zero = lab == 0;
      const float z = A.score[i];
      if (classifier) {
        counted = lab > -1;
        sc = 1.0f / (1.0f + expf(-z));
      } else {
        counted = A.label_mask[i * A.ld_label_mask] > 0.f;
        sc = z;
      }
    }
    one = one && counted, zero = zero && counted;
#pragma unroll
    for (int j = 0; j < GGNN_METRIC_MAX_THR; ++j) {
      if (j >= A.n_thr) continue;
      const float t = A.thr[j];
      const bool pos = classifier ? sc > t : sc < t, neg = classifier ? sc <= t : sc >= t;
      tp[j] += (unsigned)__popcll(__ballot(one && pos));
      fp[j] += (unsigned)__popcll(__ballot(zero && pos));
      fn[j] += (unsigned)__popcll(__ballot(one && neg));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < GGNN_METRIC_MAX_THR; ++j) {
      cnt[wave][j] = tp[j];
      cnt[wave][GGNN_METRIC_MAX_THR + j] = fp[j];
      cnt[wave][2 * GGNN_METRIC_MAX_THR + j] = fn[j];
    }
  }
  __syncthreads();

  // ---- the workgroup's row of the workspace: word t < 8 a double, word 8 + c an int64 count; waves in index order ----
  double* ws_f = reinterpret_cast<double*>(A.workspace);
  long long* ws_i = reinterpret_cast<long long*>(A.workspace);
  const int t = threadIdx.x;
  if (t < MT_F64) {
    double v = 0.0;
    for (int w = 0; w < MT_WAVES; ++w) v += red[w][t];
    ws_f[(int64_t)blockIdx.x * MT_ROW + t] = v;
  } else if (t < MT_ROW) {
    long long v = 0;
    for (int w = 0; w < MT_WAVES; ++w) v += cnt[w][t - MT_F64];
    ws_i[(int64_t)blockIdx.x * MT_ROW + t] = v;
  }
  __threadfence();
  __syncthreads();
  unsigned* counter = reinterpret_cast<unsigned*>(ws_i + (int64_t)GGNN_METRIC_BLOCKS * MT_ROW);
  if (t == 0) is_last = atomicAdd(counter, 1u) == GGNN_METRIC_BLOCKS - 1;
  __syncthreads();
  if (!is_last) return;
  __threadfence();
  // the last workgroup to arrive: thread t adds word t of every row, rows in index order, INTO the accumulator
  double* acc_f = reinterpret_cast<double*>(A.acc);
  long long* acc_i = reinterpret_cast<long long*>(A.acc) + GGNN_METRIC_F64_SLOTS;
  if (t < MT_F64) {
    double sum = 0.0;   // (device-scope loads: the other workgroups' rows come from L2)
    for (int b = 0; b < GGNN_METRIC_BLOCKS; ++b) sum += __hip_atomic_load(ws_f + b * MT_ROW + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t < GGNN_METRIC_MAX_TERMS || A.with_norm) acc_f[t] += sum;
  } else if (t < MT_ROW) {
    long long sum = 0;
    for (int b = 0; b < GGNN_METRIC_BLOCKS; ++b) sum += __hip_atomic_load(ws_i + b * MT_ROW + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    acc_i[t - MT_F64] += sum;
  } else if (t == MT_ROW) {
    if (A.loss != nullptr) {
      acc_f[MT_F64] += (double)*A.loss;
      acc_i[MT_CNT] += 1;
    }
    *counter = 0u;
  }
}

}  // namespace ggnn

extern "C" int ggnn_metric_record(const ggnn_metric_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args || !args->acc || !args->workspace) return GGNN_EINVAL;
  const ggnn_metric_args& A = *args;
  if (A.n_terms < 0 || A.n_terms > GGNN_METRIC_MAX_TERMS || A.n_thr < 0 || A.n_thr > GGNN_METRIC_MAX_THR || A.n < 0) return GGNN_EINVAL;
  if (A.mode != GGNN_METRIC_CLASSIFIER && A.mode != GGNN_METRIC_REGRESSOR) return GGNN_EINVAL;
  for (int k = 0; k < A.n_terms; ++k) {
    if (A.n_rows[k] < 0 || A.col[k] < 0) return GGNN_EINVAL;
    if (A.n_rows[k] > 0 && (!A.pred[k] || !A.target[k] || !A.mask[k] || A.ld[k] <= A.col[k] || A.ld_mask[k] < 1)) return GGNN_EINVAL;
  }
  if (A.n > 0 && A.n_thr > 0) {   // (the kernel reads score / label only then)
    if (!A.score || !A.label) return GGNN_EINVAL;
    if (A.mode == GGNN_METRIC_REGRESSOR && (!A.label_mask || A.ld_label_mask < 1)) return GGNN_EINVAL;
  }
  ggnn_metric_args K = A;
  if (K.n_thr == 0) K.n = 0;   // (no threshold, nothing to count: the kernel does not touch score / label)
  hipLaunchKernelGGL(metric_record_kernel, dim3(GGNN_METRIC_BLOCKS), dim3(MT_THREADS), 0, (hipStream_t)stream, K);
  return launch_status();
}
