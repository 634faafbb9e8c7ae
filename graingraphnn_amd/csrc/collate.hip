// Training on device-resident mini-batches:
//   ggnn_collate_batch  = the PyG DataLoader collation (train.py:365-366: node rows concatenated, edge indices offset) of the
//                         samples a device-side cursor points at, out of arenas that hold the whole dataset, into batch
//                         buffers of capacity shape -- one launch, a pure gather and copy;
//   ggnn_reverse_slots  = the forward CSR slot of every reverse (source-grouped) CSR slot of tables that keep only the
//                         first E_kept slots (masked builds: the pad edges of such a batch are in no table).
#include "common.h"
#include "segments.h"

namespace ggnn {

constexpr int CO_THREADS = 256, CO_ITEMS = 4;   // items (4-byte words of a row array, edges of a list) per thread
constexpr int CO_MAX_JOBS = GGNN_COLLATE_MAX_ROWS + GGNN_COLLATE_MAX_LISTS;

struct CollatePlan {
  int blk_off[CO_MAX_JOBS + 1];   // first workgroup of every job: the row arrays, then the lists
};

// Every workgroup reads the cursor, the batch's sample ids and the sizes of those samples for the (at most three) kinds its
// job follows, and lays the batch's prefix sums into LDS: at most 3 x 64 loads of 8 bytes per workgroup, from tables that
// stay in the caches.  The grid is sized for the capacities: it does not depend on the batch.
__global__ __launch_bounds__(CO_THREADS) void collate_batch_kernel(const ggnn_collate_args A, const CollatePlan P) {
  __shared__ int64_t s_pre[3][GGNN_COLLATE_MAX_BATCH + 1];   // first row (edge) of every slot in the batch
  __shared__ int64_t s_base[3][GGNN_COLLATE_MAX_BATCH];      // first row (edge) of the slot's sample in the arena
  const int tid = threadIdx.x, blk = (int)blockIdx.x, B = A.batch_size;
  const int32_t cur = *A.cursor_in;
  const int64_t b = ((int64_t)cur % A.n_batches + A.n_batches) % A.n_batches;
  int job = 0;
  while (job + 1 < A.n_rows + A.n_lists && blk >= P.blk_off[job + 1]) ++job;
  const bool is_list = job >= A.n_rows;
  const ggnn_collate_rows& R = A.rows[is_list ? 0 : job];
  const ggnn_collate_list& L = A.lists[is_list ? job - A.n_rows : 0];
  const int n_k = is_list ? 3 : 1;
  const int kinds[3] = {is_list ? L.kind : R.kind, L.kind_src, L.kind_dst};
  for (int idx = tid; idx < n_k * B; idx += CO_THREADS) {
    const int q = idx / B, k = idx - q * B;
    const int64_t id = A.order[b * B + k];
    const int64_t* __restrict__ off = A.sample_off[kinds[q]];
    const bool real = id >= 0 && id < A.n_samples;
    s_base[q][k] = real ? off[id] : 0;
    s_pre[q][k + 1] = real ? off[id + 1] - off[id] : 0;
  }
  __syncthreads();
  if (tid < n_k) {
    int64_t run = 0;
    s_pre[tid][0] = 0;
    for (int k = 1; k <= B; ++k) {
      run += s_pre[tid][k];
      s_pre[tid][k] = run;
    }
  }
  __syncthreads();
  const int64_t i0 = (int64_t)(blk - P.blk_off[job]) * (CO_THREADS * CO_ITEMS) + tid;
  if (!is_list) {
    // a row array: rows of `words` 4-byte words; a sample's rows are one contiguous run in the arena and in the batch, so
    // consecutive lanes copy consecutive words on both sides (rows of 8 or 11 floats start on no 16-byte boundary, and
    // the two sides' runs start at different offsets modulo 16: dword accesses)
    const int64_t n_real = min(s_pre[0][B], R.cap) * R.words, n_all = R.cap * R.words;
#pragma unroll
    for (int t = 0; t < CO_ITEMS; ++t) {
      const int64_t i = i0 + (int64_t)t * CO_THREADS;
      if (i >= n_all) break;
      uint32_t v = R.pad_word;
      if (i < n_real) {
        const int k = seg_of(s_pre[0], B, i / R.words);   // the slot whose rows hold the item (i < n_real: inside the batch)
        v = R.src[s_base[0][k] * R.words + (i - s_pre[0][k] * R.words)];
      }
      R.dst[i] = v;
    }
    if (R.meta && blk == P.blk_off[job]) {
      for (int k = tid; k <= B; k += CO_THREADS) A.batch_off[R.kind][k] = s_pre[0][k];
      if (tid == 0) *A.count[R.kind] = s_pre[0][B];
    }
  } else {
    const int64_t n_real = min(s_pre[0][B], L.cap);
#pragma unroll
    for (int t = 0; t < CO_ITEMS; ++t) {
      const int64_t e = i0 + (int64_t)t * CO_THREADS;
      if (e >= L.cap) break;
      int64_t s = L.pad_src, d = L.pad_dst;   // a pad edge: the two reserved rows, which the masked tables skip
      if (e < n_real) {
        const int k = seg_of(s_pre[0], B, e);
        const int64_t at = s_base[0][k] + (e - s_pre[0][k]);
        s = L.src[at] + s_pre[1][k];
        d = L.src[L.ld_src + at] + s_pre[2][k];
      }
      L.dst[e] = s;
      L.dst[L.cap + e] = d;
      if (L.dst_flipped) {
        L.dst_flipped[e] = d;
        L.dst_flipped[L.cap + e] = s;
      }
    }
    if (blk == P.blk_off[job]) {
      for (int k = tid; k <= B; k += CO_THREADS) A.batch_off[L.kind][k] = s_pre[0][k];
      if (tid == 0) *A.count[L.kind] = s_pre[0][B];
    }
  }
  // the cursor moves on once every workgroup has read it (ggnn_process_schedule's ticket): the last one to get here
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    if (atomicAdd(A.sync_word, 1) == (int32_t)gridDim.x - 1) {
      *A.sync_word = 0;
      *A.cursor_out = cur < INT32_MAX ? cur + 1 : cur;
    }
  }
}

struct ReverseSlotsBatch {
  ggnn_reverse_slots_args p[GGNN_COLLATE_MAX_LISTS];
};
// inv[original edge] = forward slot, over the kept slots
__global__ __launch_bounds__(256) void reverse_slots_invert_kernel(const ReverseSlotsBatch B) {
  const ggnn_reverse_slots_args& P = B.p[blockIdx.y];
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t kept = P.E_kept ? min(max(*P.E_kept, (int64_t)0), P.E) : P.E;
  if (s >= kept) return;
  const int32_t e = P.perm[s];
  if ((uint32_t)e < (uint64_t)P.E) P.scratch[e] = (int32_t)s;
}
// r_slot[reverse slot] = inv[its original edge]; the slots behind the kept ones hold 0 (a valid index, never a stale word)
__global__ __launch_bounds__(256) void reverse_slots_gather_kernel(const ReverseSlotsBatch B) {
  const ggnn_reverse_slots_args& P = B.p[blockIdx.y];
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= P.E) return;
  const int64_t kept = P.E_kept ? min(max(*P.E_kept, (int64_t)0), P.E) : P.E;
  int32_t slot = 0;
  if (q < kept) {
    const int32_t e = P.r_perm[q];
    if ((uint32_t)e < (uint64_t)P.E) slot = P.scratch[e];
  }
  P.r_slot[q] = slot;
}

}  // namespace ggnn

extern "C" int ggnn_collate_batch(const ggnn_collate_args* args, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!args) return GGNN_EINVAL;
  const ggnn_collate_args& A = *args;
  if (!A.order || !A.cursor_in || !A.cursor_out || !A.sync_word) return GGNN_EINVAL;
  if (A.n_samples < 1 || A.n_batches < 1 || A.batch_size < 1 || A.batch_size > GGNN_COLLATE_MAX_BATCH) return GGNN_EINVAL;
  if (A.n_kinds < 1 || A.n_kinds > GGNN_COLLATE_MAX_KINDS) return GGNN_EINVAL;
  if (A.n_rows < 0 || A.n_rows > GGNN_COLLATE_MAX_ROWS || A.n_lists < 0 || A.n_lists > GGNN_COLLATE_MAX_LISTS) return GGNN_EINVAL;
  if (A.n_rows + A.n_lists < 1) return GGNN_EINVAL;
  for (int k = 0; k < A.n_kinds; ++k)
    if (!A.sample_off[k] || !A.batch_off[k] || !A.count[k] || ((uintptr_t)A.count[k] & 7)) return GGNN_EINVAL;
  auto kind_ok = [&](int k) { return k >= 0 && k < A.n_kinds; };
  CollatePlan P;
  const int64_t per_blk = CO_THREADS * CO_ITEMS;
  int64_t nblk = 0;
  for (int j = 0; j < A.n_rows; ++j) {
    const ggnn_collate_rows& R = A.rows[j];
    if (!R.src || !R.dst || R.cap < 1 || R.words < 1 || R.words > 64 || !kind_ok(R.kind) || (R.meta != 0 && R.meta != 1))
      return GGNN_EINVAL;
    P.blk_off[j] = (int)nblk;
    nblk += (R.cap * R.words + per_blk - 1) / per_blk;
    if (nblk >= (1 << 30)) return GGNN_EINVAL;
  }
  for (int j = 0; j < A.n_lists; ++j) {
    const ggnn_collate_list& L = A.lists[j];
    if (!L.src || !L.dst || L.cap < 1 || L.ld_src < 0 || !kind_ok(L.kind) || !kind_ok(L.kind_src) || !kind_ok(L.kind_dst))
      return GGNN_EINVAL;
    if (L.pad_src < 0 || L.pad_dst < 0) return GGNN_EINVAL;
    P.blk_off[A.n_rows + j] = (int)nblk;
    nblk += (L.cap + per_blk - 1) / per_blk;
    if (nblk >= (1 << 30)) return GGNN_EINVAL;
  }
  for (int j = A.n_rows + A.n_lists; j <= CO_MAX_JOBS; ++j) P.blk_off[j] = (int)nblk;
  hipLaunchKernelGGL(collate_batch_kernel, dim3((unsigned)nblk), dim3(CO_THREADS), 0, (hipStream_t)stream, A, P);
  return launch_status();
}

extern "C" int ggnn_reverse_slots(const ggnn_reverse_slots_args* lists, int n_lists, ggnn_stream_t stream) {
  using namespace ggnn;
  if (!lists || n_lists < 1 || n_lists > GGNN_COLLATE_MAX_LISTS) return GGNN_EINVAL;
  ReverseSlotsBatch B;
  int64_t max_E = 0;
  for (int k = 0; k < GGNN_COLLATE_MAX_LISTS; ++k) {
    B.p[k] = lists[k < n_lists ? k : 0];
    if (k >= n_lists) continue;
    const ggnn_reverse_slots_args& P = B.p[k];
    if (P.E < 0 || P.E >= INT32_MAX || (P.E_kept && ((uintptr_t)P.E_kept & 7))) return GGNN_EINVAL;
    if (P.E > 0 && (!P.perm || !P.r_perm || !P.r_slot || !P.scratch)) return GGNN_EINVAL;
    max_E = P.E > max_E ? P.E : max_E;
  }
  if (max_E == 0) return GGNN_OK;
  const dim3 grid((unsigned)((max_E + 255) / 256), (unsigned)n_lists);
  hipLaunchKernelGGL(reverse_slots_invert_kernel, grid, dim3(256), 0, (hipStream_t)stream, B);
  hipLaunchKernelGGL(reverse_slots_gather_kernel, grid, dim3(256), 0, (hipStream_t)stream, B);
  return launch_status();
}
