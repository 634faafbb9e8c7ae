/*
 * ggnn.h -- C ABI of libggnn.so: the MI355X (gfx950) kernels behind the GrainGNN rollout
 * hot path (GrainNN_regressor.forward + GrainNN_classifier.forward + rollout-step glue).
 *
 * Every entry point is `extern "C"`, takes raw DEVICE pointers + sizes + a hipStream_t
 * (passed as void*), never allocates, never synchronises, never throws, keeps no global
 * state, and returns 0 or a negative GGNN_E* code.  All work is enqueued on `stream`, so
 * a caller may capture any sequence of calls into a hipGraph.
 *
 * Citations (file:line) are into the reference repository YigongQin/GrainGraphNN.  The
 * reference has no FFI of its own (it is pure Python on PyTorch + PyG); each entry point
 * names the Python function(s) whose work it replaces.  INTEGRATION.md shows the ctypes
 * binding a reference maintainer would add.
 *
 * Fixed by the shipped models (parameters.py:18-50, 97-134): hidden width C = 96, one
 * attention head, fp32 everywhere.  Features per node <= 12 (grain 11, joint 8).
 */
#ifndef GGNN_H_
#define GGNN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GGNN_ABI_VERSION 26
#define GGNN_C 96              /* hidden width (hyper.layer_size of every shipped model) */
#define GGNN_MAX_GATES 4       /* i, f, c, o */
#define GGNN_EDGE_PARAM_ROWS 3 /* per gate: W_value[:, 0:3] (the value side of the min-image correction) */
#define GGNN_UNIT_EDGES 3      /* in-edges per aggregation unit (every junction has exactly 3) */

#define GGNN_OK 0
#define GGNN_EINVAL (-1)  /* bad argument (null pointer, size, alignment, unsupported width) */
#define GGNN_ELAUNCH (-2) /* hipLaunch / hipMemsetAsync reported an error */
#define GGNN_ETOPOLOGY (-3) /* ggnn_topology_update: the lists are not a valid grain graph (message in args->error) */

typedef void* ggnn_stream_t; /* hipStream_t */

/* Gate-epilogue modes of ggnn_lstm_epilogue_batch */
#define GGNN_MODE_LSTM 0    /* 4 gates (i,f,c,o), c_in given: c' = f*c + i*tanh(.), h' = o*tanh(c') */
#define GGNN_MODE_LSTM_H0 1 /* 3 gates (i,c,o), h = c = 0 (encoder): c' = i*tanh(.), h' = o*tanh(c') */
#define GGNN_MODE_RAW 2     /* no LSTM: write the n_gates pre-activations (used for PeriodConv parity) */

int ggnn_version(void);
const char* ggnn_error_string(int code);
/* Arithmetic of the K >= 100 GEMMs (decoder ggnn_project_batch, ggnn_lstm_epilogue_batch), fixed per process
 * by the environment variable GGNN_GEMM: GGNN_GEMM_BF16X6 (default) = every fp32 operand split
 * exactly into three bf16 pieces, six bf16 MFMA products per k-step, fp32 accumulate (dropped
 * terms <= 2^-25 of a product: fp32-equivalent); GGNN_GEMM_FP32 ("fp32") = native fp32 MFMA. */
#define GGNN_GEMM_FP32 0
#define GGNN_GEMM_BF16X6 1
int ggnn_gemm_mode(void);

/* ------------------------------------------------------------------------------------
 * CSR build.  Replaces the COO bookkeeping inside PyG MessagePassing.propagate as used at
 * periodGATconv.py:174-175 (gather by edge_index[0]/[1], scatter-add by edge_index[1]):
 * edges are grouped by destination once per topology, so aggregation needs no atomics.
 * One to four lists per call, in one sequence of seven launches (a topological event rebuilds
 * the three edge types' tables).  Per list (ggnn_csr_args):
 *   edge_index : [2, E] int64, row 0 = source node, row 1 = destination node (device)
 *   rowptr     : [n_dst + 1] int32 out
 *   col        : [E] int32 out, source node of each CSR slot
 *   perm       : [E] int32 out, original COO edge id of each CSR slot (ascending inside a
 *                row => the result is deterministic and order-stable)
 *   row        : [E] int32 out, destination node of each CSR slot
 *   unit_ptr   : [n_dst + 1] int32 out, first unit of every destination row
 *   units      : [ggnn_csr_max_units(E, n_dst), 8] int32 out, 16-byte aligned.  A unit is a
 *                destination row restricted to <= GGNN_UNIT_EDGES consecutive in-edges:
 *                {i, p0, nact | first<<8 | last<<9, 0, j0, j1, j2, 0}; rows without edges
 *                get one empty unit; absent edges repeat j0.  unit_ptr[n_dst] = #units.
 *   flags      : [1] int32 device word, bit 0 is OR-ed in when an index is out of range
 *                (such edges are dropped; the host wrapper raises)
 *   workspace  : ggnn_csr_workspace_bytes(E, n_dst) bytes of device scratch
 */
size_t ggnn_csr_workspace_bytes(int64_t E, int64_t n_dst);
int64_t ggnn_csr_max_units(int64_t E, int64_t n_dst); /* upper bound: n_dst + E / GGNN_UNIT_EDGES */
typedef struct ggnn_csr_args {
  const int64_t* edge_index;
  int64_t E, n_src, n_dst;
  int32_t* rowptr;
  int32_t* col;
  int32_t* perm;
  int32_t* row;
  int32_t* unit_ptr;
  int32_t* units;
  int32_t* flags;
  void* workspace;
  size_t workspace_bytes;
} ggnn_csr_args;
/* A mask (no-flux boundary): the tables of the list WITHOUT every edge whose source equals skip_src or whose destination
 * equals skip_dst (-1 = none) -- the copies of test.py:363-375 that both forwards see when grain 0 is the boundary grain
 * (skip_src = 0 for grain->joint, skip_dst = 0 for joint->grain).  Inside a row the slots stay in original-edge order (the
 * order `index[:, mask]` produces); perm maps every slot to its edge id in the FULL list, so ggnn_edge_prepare reads the
 * full list's edge_attr and writes the filtered records.  The kept slots are [0, rowptr[n_dst]); the rest of col / perm /
 * row up to E is written with zeros.  An in-place refill of the same tables (the event loop) passes the same mask again. */
typedef struct ggnn_csr_mask {
  int64_t skip_src, skip_dst;
  int64_t* E_kept; /* NULL, or an 8-byte aligned int64 device word that receives rowptr[n_dst]: the E_dev of the per-edge
                      kernels (ggnn_prepare_edge.E_dev) that read this table, whose launches are sized for E */
} ggnn_csr_mask;
int ggnn_build_csr_batch(const ggnn_csr_args* problems, const ggnn_csr_mask* masks /* [n_problems], or NULL: no list masked */,
                         int n_problems, ggnn_stream_t stream);
/* Masked tables of a disjoint union of n_traj trajectories (a no-flux ensemble: every trajectory has a boundary grain of its
 * own, its local grain 0).  Per list a ggnn_csr_union: src_off / dst_off = [n_traj + 1] int64 device offsets of the source /
 * destination node type, rising from 0 to the node count (equal offsets: an empty trajectory), or NULL: that side is not
 * split.  The list's skip_src / skip_dst then mean LOCAL indices on the sides that are split: an edge is left out when
 * s - src_off[traj(s)] == skip_src or d - dst_off[traj(d)] == skip_dst, traj(v) = the last trajectory whose offset is <= v
 * (with skip 0: the node is one of the offsets of a trajectory that has nodes).  Tables, slot order, perm into the FULL list
 * and E_kept as above.  unions == NULL, or both pointers NULL: ggnn_build_csr_batch. */
typedef struct ggnn_csr_union {
  const int64_t* src_off;
  const int64_t* dst_off;
  int64_t n_traj;
} ggnn_csr_union;
int ggnn_build_csr_batch_traj(const ggnn_csr_args* problems, const ggnn_csr_mask* masks,
                              const ggnn_csr_union* unions /* [n_problems], or NULL */, int n_problems, ggnn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Per-edge record in CSR order, computed once per forward and shared by every gate of the
 * encoder and decoder cells (GGNN_EINFO_ROW = 20 floats per edge):
 *   einfo[p, 0..15]  = (reloc_xyz, x_src[col[p], 3 .. f_src), 0.., 1 at 12, edge_attr at 13, 0, 0)
 *                      -- the non-hidden part of the source row the attention score is taken with;
 *                      when f_src <= 11 slot 11 is 1 as well (the bias row of the encoder sweep's
 *                      value product; the score tail u4 is 0 there)
 *   einfo[p, 16..19] = (reloc_x, reloc_y, reloc_z, edge_attr)
 * with reloc = min-image(x_src[col[p], :3] - x_dst[row[p], :3]) exactly as periodGATconv.py:209-210
 * (rel > 0.5 -> rel - 1, rel < -0.5 -> rel + 1) and edge_attr taken from the ORIGINAL COO
 * order through perm (edge_attr_dict[et][:, 0]).  Up to three edge types per launch.
 */
#define GGNN_EINFO_ROW 20
typedef struct ggnn_prepare_edge {
  const int32_t* col;     /* [E] */
  const int32_t* perm;    /* [E] */
  const int32_t* row;     /* [E] */
  const float* edge_attr; /* [E] COO order */
  const float* x_src;     /* [n_src, ldx_src] */
  const float* x_dst;     /* [n_dst, ldx_dst] */
  float* einfo;           /* [E + GGNN_UNIT_EDGES, GGNN_EINFO_ROW] out, 16-byte aligned (tail rows are padding) */
  int64_t ldx_src, ldx_dst, E, f_src; /* 3 <= f_src <= 12 source features */
  const int64_t* E_dev;   /* NULL, or the number of edges read from DEVICE memory when the kernel runs (E is then the
                             capacity the launch is sized for, *E_dev <= E) -- a launch captured in a hipGraph follows an
                             edge list that SHRINKS in place (GrainRollout's event loop: grain eliminations remove edges;
                             the lists, CSR tables and per-edge buffers keep their addresses and capacity) */
} ggnn_prepare_edge;
int ggnn_edge_prepare(const ggnn_prepare_edge* edges, int n_edge_types, ggnn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Node-level projection: out[M, ncols] = [X[:, :F] | H] . Wp^T + bias.
 * Replaces, for all gates and edge types at once, the per-edge lin_query / lin_key /
 * lin_value (periodGATconv.py:216-218) and lin_skip (:186) applied to cat[x, h]
 * (heteropgclstm.py:112,120,128,137), using linearity to hoist them from edges to nodes.  What
 * the rows of Wp hold is the caller's business (graingraphnn_amd/packing.py: value rows for the
 * node as a source; W_k^T W_q / sqrt(96) rows for it as a destination, see
 * ggnn_period_gat_aggregate_batch; summed skip rows).
 *   X  : [M, ldx] node features, first F columns used (F <= 12)
 *   H  : [M, ldh] hidden state (k2 = 96) or NULL (k2 = 0, encoder: h = 0)
 *   Wp : [ncols, Kp] packed weight rows, Kp = roundup4(F) + k2; columns [F, roundup4(F)) zero
 *   ncols % 96 == 0; ldo % 4 == 0; H, Wp, bias, out 16-byte aligned.
 * One to four projections per launch: the node types of one cell and / or the same cell of the
 * regressor and the classifier (both see the same x_dict, test.py:382-383).  All problems must share
 * k2.  Rows are addressed with a 64-bit tile base and 32-bit offsets inside a 16-row tile:
 * 16 * max(ldx, ldh, ldo) < 2^31 is the only size limit.
 */
typedef struct ggnn_project_args {
  const float* X;
  const float* H; /* NULL when k2 == 0 */
  const float* Wp;
  const float* bias;
  float* out;
  int64_t ldx, ldh, M, ldo;
  int32_t F, k2, ncols;
  int32_t precision; /* 0: fp32-equivalent over fp32's whole range (exact 3-piece bf16 split, 6 products per k-step);
                        GGNN_PRECISION_F16X2 (k2 == 96 only): fp32-equivalent for |x|, |h|, |w| < 65504 -- the fused
                        cells' arithmetic, two fp16 pieces per operand and THREE products per k-step (operands beyond
                        the range are clamped: the caller checks its weights, packing.pack_cell; the node rows are the
                        ones ggnn_decoder_cell_batch checks and reports) -- the value rows of the fused decoder plan;
                        GGNN_PRECISION_BF16 (k2 == 96 only): operands rounded to bf16, ONE bf16 MFMA product per
                        k-step, fp32 accumulate -- what torch.autocast(bfloat16) asks of a linear (training path).
                        | GGNN_OUT_BLOCK_MAJOR (k2 == 96 only): `out` is [ncols / 96][M][96] -- every block of 96
                        columns a contiguous [M, 96] matrix of its own (ldo is ignored) -- instead of [M, ldo]: the layout
                        of the fused decoder plan's value rows, which are written once here and gathered 96 columns
                        (one edge type and gate) at a time by ggnn_decoder_cell_batch (v_block_major) */
} ggnn_project_args;
int ggnn_project_batch(const ggnn_project_args* args, int n_problems, ggnn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Periodic-boundary GAT aggregation for one edge type, all gates fused.  Replaces
 * PeriodConv.message (periodGATconv.py:204-236) + PyG propagate's gather and scatter-add:
 * min-image wrap of the first three coordinates, scaled dot of query and key, segment softmax
 * (+1e-16), relu of the value, alpha-weighted sum.  The key is never formed: with
 * x~_j = [reloc_e, x_j[3:F], h_j] the score q_i.(W_k x~_j + b_k + w_edge a_e)/sqrt(96) equals
 * u_i . x~_j + s1_i + a_e s2_i, where u_i = W_k^T q_i/sqrt(96), s1_i = b_k.q_i/sqrt(96) and
 * s2_i = w_edge.q_i/sqrt(96) are affine in the destination's [x_i | h_i] and come from
 * ggnn_project_batch.  Per destination i and gate g the projections hold
 *   p_dst[i, u_off  + g*96 + 0..95] = u_i[F ..]   (hidden-state part; absent when h_src == NULL)
 *   p_dst[i, u4_off + g*16 + 0..15] = (u_i[0..F-1], 0.., s1_i at 12, s2_i at 13, 0, 0), dotted
 *                                     with einfo[e, 0..15]
 *   p_src[j, v_off  + g*96 + 0..95] = lin_value(x_j with its first three columns zeroed, h_j)
 * and the sweep writes
 *   agg[i, g*a_gstride + a_off + 0..95] = sum_e alpha_e * relu(lin_value(x~_j))
 *   agg[i, g*a_gstride + sc_off + 0]    = sum_e alpha_e            (1, or 0 if no in-edge)
 *   agg[i, g*a_gstride + sc_off + 1]    = sum_e alpha_e * edge_attr_e
 * (lin_l2, its bias, the value-side lin_edge term and lin_skip are applied afterwards by
 * ggnn_lstm_epilogue_batch, which is exact because they are linear in these sums.)
 */
typedef struct ggnn_aggregate_args {
  const int32_t* unit_ptr;  /* [n_dst + 1] from ggnn_build_csr_batch */
  const int32_t* units;     /* [n_units, 8] from ggnn_build_csr_batch */
  const float* einfo;       /* [E + GGNN_UNIT_EDGES, GGNN_EINFO_ROW] from ggnn_edge_prepare */
  const float* p_src;       /* [n_src, ldp_src] projections of the source node type */
  const float* p_dst;       /* [n_dst, ldp_dst] projections of the destination node type */
  const float* h_src;       /* [n_src, ldh_src] source hidden state, or NULL (encoder: h = 0) */
  const float* edge_params; /* [n_gates][GGNN_EDGE_PARAM_ROWS][96] = W_value[:, 0..2] */
  float* agg;               /* [n_dst, ld_agg] */
  int64_t ldp_src, ldp_dst, ld_agg, ldh_src, n_src, n_dst, E;
  int32_t v_off, u_off, u4_off, a_off, a_gstride, sc_off, n_gates;
  int32_t pad_n;            /* the sweep also writes zeros into agg[i, g a_gstride + sc_off + 2 .. + pad_n) of every gate
                               row (the padding between the last edge type's scalars and the next gate row, which the training
                               path's gate GEMM multiplies with zero weight columns: it has to be finite); 0 = nothing */
} ggnn_aggregate_args;
/* The 1..6 sweeps of one cell (HeteroConv over the edge types, heteropgclstm.py:148-183; of one
 * model, or of the regressor and the classifier, which see the same graph: test.py:382-383) in ONE
 * launch: args[0..n_sweeps).  All must have the same n_gates and agree on h_src == NULL; they may
 * write disjoint columns of the same agg rows. */
int ggnn_period_gat_aggregate_batch(const ggnn_aggregate_args* args, int n_sweeps,
                                    ggnn_stream_t stream);

/* Encoder form of the sweep (h = c = 0, heteropgclstm.py:101-110 with the zero state of
 * models.py:422: the cell sees the bare features), values on the matrix cores: nothing is gathered
 * from a projected source row.  With h = 0 the value of an edge is relu(W_value . [reloc, x_j[3:F]]
 * + b_value), a product of the edge's own einfo record, so p_src / v_off / edge_params of
 * ggnn_aggregate_args are replaced by
 *   wv_frag: [6 * n_gates][3][64] fp32, MFMA B fragments of Bp [12, n_gates * 96] with
 *            Bp[k][g*96 + ch] = W_value_g[ch][k] for k < F_src (columns 0..2 act on reloc),
 *            Bp[11][.] = b_value_g, 0 elsewhere (F_src <= 11; einfo[:, 11] = 1):
 *            element [t][s][l] = Bp[4 s + (l >> 4)][(t / 6) * 96 + 32 ((t % 6) / 2) + 2 (l & 15) + t % 2].
 * p_dst, u4_off, agg, a_off, a_gstride, sc_off and the result are those of the h_src == NULL form
 * of ggnn_period_gat_aggregate_batch (same sums up to fp32 re-association).  n_gates = 3; a_off, a_gstride,
 * ld_agg even.  Up to six sweeps per launch (three edge types x two models). */
typedef struct ggnn_aggregate_enc_args {
  const int32_t* unit_ptr; /* [n_dst + 1] from ggnn_build_csr_batch */
  const int32_t* units;    /* [n_units, 8] from ggnn_build_csr_batch */
  const float* einfo;      /* [E + GGNN_UNIT_EDGES, GGNN_EINFO_ROW] from ggnn_edge_prepare */
  const float* p_dst;      /* [n_dst, ldp_dst] destination projections (the u4 tails) */
  const float* wv_frag;    /* [6 * n_gates][3][64] */
  float* agg;              /* [n_dst, ld_agg] */
  int64_t ldp_dst, ld_agg, n_dst, E;
  int32_t u4_off, a_off, a_gstride, sc_off, n_gates, reserved;
} ggnn_aggregate_enc_args;
int ggnn_period_gat_aggregate_enc_batch(const ggnn_aggregate_enc_args* args, int n_sweeps,
                                        ggnn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Backward of one sweep (training path).  Replaces what autograd does for
 * PeriodConv.message + propagate (periodGATconv.py:174-175, 204-236) in train.py:158-166:
 * segment-softmax backward, relu mask, scatter of the value / hidden-state gradients to the
 * source rows -- without atomics (a destination-grouped pass, then a source-grouped pass over
 * the reverse CSR), so gradients are reproducible run to run.
 * Forward operands exactly as in ggnn_aggregate_args (same offsets and strides) plus the saved
 * forward output `agg` and the incoming gradient `g_agg` (same layout as agg; only the 96 value
 * columns and the two scalars of every gate are read).  Outputs, in the layout of their operand:
 *   g_p_dst[i, u_off + g*96 ..], g_p_dst[i, u4_off + g*16 ..]   (other columns untouched)
 *   g_p_src[j, v_off + g*96 ..]                                  (other columns untouched)
 *   g_h_src[j, 0..95]                                            (when h_src != NULL)
 *   ep_partial[w, g, k, c]: partial sums of d edge_params; the gradient is their sum over w.
 * The geometry (einfo) carries no gradient through this entry point; ggnn_period_gat_aggregate_backward_inputs below
 * adds the gradient of the edge records, i.e. of the node features and of the edge attribute they were made from.
 */
typedef struct ggnn_aggregate_bwd_args {
  const int32_t* rowptr;   /* [n_dst + 1] destination-grouped CSR (ggnn_build_csr_batch) */
  const int32_t* col;      /* [E] source node of every CSR slot */
  const float* einfo;      /* [E + GGNN_UNIT_EDGES, GGNN_EINFO_ROW] */
  const float* p_src;      /* forward operands, as ggnn_aggregate_args */
  const float* p_dst;
  const float* h_src;      /* or NULL */
  const float* edge_params;
  const float* agg;        /* [n_dst, ld_agg] forward output */
  const float* g_agg;      /* [n_dst, ld_agg] gradient with respect to agg */
  const int32_t* r_rowptr; /* [n_src + 1] source-grouped (reverse) CSR of the same edges */
  const int32_t* r_dst;    /* [E] destination node of every reverse slot */
  const int32_t* r_slot;   /* [E] forward CSR slot of every reverse slot */
  float* edge_alpha;       /* [E, n_gates] scratch: attention weights */
  float* edge_ds;          /* [E, n_gates] scratch: score gradients */
  float* ep_partial;       /* [n_partials, n_gates, 3, 96] out */
  float* g_p_dst;          /* [n_dst, ldp_dst] out */
  float* g_p_src;          /* [n_src, ldp_src] out */
  float* g_h_src;          /* [n_src, ldh_src] out, or NULL */
  int64_t ldp_src, ldp_dst, ld_agg, ldh_src, n_src, n_dst, E, n_partials;
  int32_t v_off, u_off, u4_off, a_off, a_gstride, sc_off, n_gates;
  int32_t g_h_accumulate;  /* 1 = g_h_src += (the sweeps of a cell that share a source node type add into one buffer
                              the first of them wrote), 0 = g_h_src is written */
} ggnn_aggregate_bwd_args;
int64_t ggnn_aggregate_bwd_partials(int64_t n_dst); /* rows of ep_partial the call writes (one per workgroup of its destination pass) */
int ggnn_period_gat_aggregate_backward(const ggnn_aggregate_bwd_args* args, ggnn_stream_t stream);

/* The same backward with the gradients of the sweep's INPUTS: everything ggnn_period_gat_aggregate_backward
 * writes, bit for bit, plus the gradient of the edge records einfo[p] = (x4 [16] | reloc [3] | a) mapped back through the
 * record's column map (GGNN_EINFO_ROW above).  Per CSR slot p (edge j -> i), summed over the gates:
 *   g_x4[p, k] = sum_g ds u4_i[k]                                     k = 0..15
 *   g_r[p, k]  = sum_g sum_c alpha g_out_i[c] [val[c] > 0] W3_g[k, c]  k = 0..2
 *   g_a[p]     = g_x4[p, 13] + sum_g alpha g_sae_i
 * The min-image shift is piecewise constant, so with g_reloc = g_x4[p, 0..2] + g_r[p]:
 *   g_x_src[j, 0..2] += g_reloc      g_x_dst[i, 0..2] -= g_reloc      g_x_src[j, 3..f_src-1] += g_x4[p, 3..f_src-1]
 *   g_edge_attr[perm[p]] = g_a[p]    (perm is a permutation of the list's edges: every entry written once; entries of
 *                                     edges a masked table leaves out are not written)
 * Columns 12, 11 (f_src <= 11) and the padding of the record are constants.  Atomics-free and in a fixed order: the
 * destination pass writes edge_grad and g_x_dst (one wave per row), a third launch gathers edge_grad over the reverse
 * CSR (16 lanes per source row); the source pass is the one of ggnn_period_gat_aggregate_backward.  The *_accumulate
 * flags add to what the buffer holds (a node type is the source and the destination of several sweeps of a cell: the
 * calls of one stream are ordered); 0 writes columns 0..2 (dst) / 0..f_src-1 (src) of every row. */
typedef struct ggnn_aggregate_bwd_inputs {
  const int32_t* perm;   /* [E] edge id of every CSR slot in the caller's list (ggnn_build_csr_batch) */
  float* edge_grad;      /* [max(E, 1), 16] scratch: gradient of the record's first 16 columns, g_r folded into 0..2, g_a at 13 */
  float* g_x_src;        /* [n_src, ldgx_src] out */
  float* g_x_dst;        /* [n_dst, ldgx_dst] out (may be g_x_src when the two node types are one) */
  float* g_edge_attr;    /* [edges of the caller's list] out */
  int64_t ldgx_src, ldgx_dst;
  int32_t f_src;         /* 3 <= f_src <= 12, as ggnn_prepare_edge.f_src */
  int32_t g_x_src_accumulate, g_x_dst_accumulate, reserved;
} ggnn_aggregate_bwd_inputs;
int ggnn_period_gat_aggregate_backward_inputs(const ggnn_aggregate_bwd_args* args, const ggnn_aggregate_bwd_inputs* inputs,
                                              ggnn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Gate GEMM + LSTM epilogue (arithmetic per ggnn_gemm_mode).  For every node and gate:
 *   pre[g] = agg[:, g, 0:Ka] . W2[g]^T + p_dst[:, s_off + g*96 ...]
 * where W2[g] = [lin_l2.weight of each incoming edge type | b_l2, w_edge per edge type]
 * (periodGATconv.py:218, 231-235), the skip/bias term was produced by ggnn_project_batch
 * (lin_skip summed over incoming edge types = HeteroConv aggr 'sum', plus b_{i,f,c,o}),
 * followed by the cell update of heteropgclstm.py:111-146.
 *   mode GGNN_MODE_LSTM    : n_gates = 4, needs c_in, writes h_out, c_out   [N, 96]
 *   mode GGNN_MODE_LSTM_H0 : n_gates = 3 (i, c, o), writes h_out, c_out
 *   mode GGNN_MODE_RAW     : writes raw_out [N, n_gates*96] = pre
 * Ka % 4 == 0, Ka <= 200.
 * One to four problems per launch: the node types of one cell (heteropgclstm.py:111-146 runs the
 * update per node type) and / or the same cell of the regressor and the classifier (test.py:382-383
 * calls both models on the same x_dict).  All problems must share `mode` and `n_gates`; Ka may differ.
 */
typedef struct ggnn_epilogue_args {
  const float* agg;   /* [N, n_gates*Ka] */
  const float* w2;    /* [n_gates][96][Ka] */
  const float* p_dst; /* [N, ldp] */
  const float* c_in;  /* [N, 96] or NULL */
  float* h_out;       /* [N, 96] */
  float* c_out;       /* [N, 96] */
  float* raw_out;     /* [N, n_gates*96] (GGNN_MODE_RAW) */
  int64_t ldp, N;
  int32_t Ka, s_off, n_gates, mode;
  /* Optional (NULL = native fp32 MFMA kernel): w2[:, :, 0:Ka-4] re-ordered into MFMA A fragments,
   * fp32, [n_gates][(Ka-4)/32][6][2][64][4]: element [g][ks][ct][h][l][j] =
   * w2[g][16 ct + (l & 15)][32 ks + 8 (l >> 4) + 4 h + j] (one 16-byte load per lane of a wave =
   * 1 KB of contiguous memory).  The kernel splits every value exactly into three bf16 pieces
   * (x = hi + mid + lo, each the bf16 round-to-nearest of what is left) on the fly.  16-byte
   * aligned; declared as uint16 pairs for historical reasons (ABI <= 12 passed pre-split planes).
   * Used when ggnn_gemm_mode() == GGNN_GEMM_BF16X6; Ka - 4 must be a multiple of 32. */
  const uint16_t* w2_planes;
  /* Layout of agg: row stride ld_agg and gate stride g_stride, in floats (0, 0 = packed:
   * g_stride = Ka, ld_agg = n_gates * Ka).  Both multiples of 4, g_stride >= Ka,
   * ld_agg >= n_gates * g_stride.  Multiples of 32 (128-byte aligned k-steps) are what the
   * workspace uses: the fragment loads of the bf16x6 kernel then touch one cache line each. */
  int64_t ld_agg;
  int32_t g_stride, reserved;
} ggnn_epilogue_args;
int ggnn_lstm_epilogue_batch(const ggnn_epilogue_args* args, int n_problems, ggnn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Encoder cell (h = c = 0; HeteroPGCLSTM.forward on the zero state of models.py:422,
 * heteropgclstm.py:101-183: no forget gate) with EVERYTHING that belongs to a destination node in one kernel and
 * one launch: the score tails u4, the sweeps of the incoming edge types (PeriodConv.message,
 * periodGATconv.py:204-236), lin_l2 + the lin_edge value term, HeteroConv's sum over the edge types
 * (heteropgclstm.py:113-138), the summed skip term and the LSTM update.  Replaces the encoder's share of
 * ggnn_project_batch, ggnn_period_gat_aggregate_enc_batch and ggnn_lstm_epilogue_batch(GGNN_MODE_LSTM_H0) -- same
 * sums up to fp32 re-association; nothing but x, the edge records and the weights is read, nothing but (h, c) is
 * written.  One problem = one destination node type of one model, with its 1 or 2 incoming edge types; up to four
 * problems (two node types x regressor and classifier, test.py:382-383) per call.
 *
 * With h = 0 a PeriodConv only sees 16-slot rows: of a destination node (x_0 .. x_{f_dst-1}, 0 .., 1 at slot 12)
 * and of an in-edge (ggnn_edge_prepare's record: reloc, x_src[3 .. f_src), 0 .., 1 at 12, edge length at 13).
 * A workgroup of eight waves owns 128 consecutive destination nodes, one 16-node tile per wave, and walks the
 * gates i, c~, o; per gate g and incoming edge type e: u4[node] = T(e, g) . feature slots; score of an in-edge =
 * u4[node] . record; online-max softmax over the node's in-edges (PyG: exp(s - max) / (sum + 1e-16)); value of an
 * in-edge = relu(V(e, g) . record) (its row 12 column is b_value); aggregate = sum alpha value; pre-activation +=
 * lin_l2(e, g) . aggregate + b_l2 sum alpha + w_edge sum alpha a_e; then + S(g) . feature slots (summed lin_skip +
 * gate bias); i = sig, c' = i tanh(c~), h' = sig(o) tanh(c').  Arithmetic and OPERAND RANGE as for
 * ggnn_decoder_cell_batch (two fp16 pieces, three products; |x| < 65504, reported through *flags).
 *
 * Per incoming edge type: rowptr [n_dst + 1] (ggnn_build_csr_batch), einfo (ggnn_edge_prepare), E.
 * Per problem:
 *   x_dst   : [n_dst, ldx] features of the destination nodes (first f_dst <= 12 columns)
 *   wstream : the weight slices in the order the kernel consumes them (packing.encoder_cell_stream):
 *             for g in (i, c~, o): for e: 1 slice A(e, g) | 3 slices lin_l2(e, g); then 1 slice S(g).
 *             Every slice is GGNN_DC_SLICE_BYTES in ggnn_dec_cell_args.wstream's image
 *             ([column tile nb][plane hi, lo'][64 lanes][8 fp16], lane l = 16 kq + m of (nb, plane) holds
 *             W[16 nb + m][32 ks + 8 kq .. + 7]).  A(e, g) = [V(e, g) rows 0..95 | T(e, g) rows 96..111] and S(g)
 *             [96 rows] are ONE k-step over the 16 slots: k = 8 q + j holds slot 4 q + j for j < 4 and zero for
 *             j >= 4.  lin_l2(e, g) is [96 x 96] in three k-steps, column k = the lin_l2 column of aggregate
 *             channel GGNN_CELL_P3_CHANNEL(k).
 *   w2_tail : [3][n_in][6][64] fp32: (b_l2, w_edge) of (g, e) as v_mfma_f32_16x16x4_f32 A fragments
 *             ([ct][l]: k = l >> 4; k = 0 -> b_l2[16 ct + (l & 15)], k = 3 -> w_edge[16 ct + (l & 15)], else 0)
 *   h_out, c_out : [n_dst, 96]
 *   flags   : optional int32 device word (GGNN_FLAG_F16_RANGE) */
/* column k = 32 ks + 8 kq + j of a lin_l2 block <-> aggregate channel 32 ks + 16 (j / 4) + 4 kq + j % 4 */
#define GGNN_CELL_P3_CHANNEL(k) (32 * ((k) / 32) + 16 * (((k) % 8) / 4) + 4 * (((k) % 32) / 8) + (k) % 4)
typedef struct ggnn_enc_cell_sweep {
  const int32_t* rowptr;   /* [n_dst + 1] */
  const float* einfo;      /* [E + GGNN_UNIT_EDGES, GGNN_EINFO_ROW] */
  int64_t E;
} ggnn_enc_cell_sweep;
typedef struct ggnn_enc_cell_args {
  ggnn_enc_cell_sweep in[2];
  const float* x_dst;   /* [n_dst, ldx] */
  float* h_out;         /* [n_dst, 96] */
  float* c_out;         /* [n_dst, 96] */
  const void* wstream;  /* [3 * (4 n_in + 1)][GGNN_DC_SLICE_BYTES] */
  const float* w2_tail; /* [3][n_in][6][64] */
  int32_t* flags;       /* optional */
  int64_t n_dst, ldx;
  int32_t n_in, f_dst;
} ggnn_enc_cell_args;
int ggnn_encoder_cell_batch(const ggnn_enc_cell_args* args, int n_problems, ggnn_stream_t stream);

/* The encoder cell of ggnn_encoder_cell_batch (same h_out, c_out, flags, bit for bit) with the DECODER's source-side
 * value rows of the same node type as an epilogue: V = [x | h_out] . Wv^T + bv, the rows ggnn_project_batch writes
 * with GGNN_PRECISION_F16X2 | GGNN_OUT_BLOCK_MAJOR (same two-piece, three-product arithmetic, the bias as one more
 * product against the constant slot), so the decoder cell reads them where it always does.
 *   vstream : [4 n_blocks][GGNN_DC_SLICE_BYTES] (packing.encoder_values_stream): per 96-column block b, three k-steps
 *             over h (column k = 32 ks + 8 kq + j <-> h channel GGNN_CELL_P3_CHANNEL(k)) and one over the 16 feature
 *             slots (as A(e, g) above: x_0 .. x_{f_dst-1}, slot 12 = bv, the rest zero) -- 6 column tiles per slice
 *   v_out   : [n_blocks][n_dst][96], 16-byte aligned
 *   n_blocks: 1 .. GGNN_ENC_VALUES_MAX_BLOCKS
 * Range: h_out is below 1 in magnitude; x is covered by the cell's own flag; the weights are checked when packed. */
#define GGNN_ENC_VALUES_MAX_BLOCKS 8
typedef struct ggnn_enc_values_args {
  ggnn_enc_cell_args cell;
  const void* vstream;  /* [4 n_blocks][GGNN_DC_SLICE_BYTES] */
  float* v_out;         /* [n_blocks][n_dst][96] */
  int32_t n_blocks;
  int32_t reserved;
} ggnn_enc_values_args;
int ggnn_encoder_cell_values_batch(const ggnn_enc_values_args* args, int n_problems, ggnn_stream_t stream);

/* Decoder HeteroPGCLSTM cell (h, c from the encoder; heteropgclstm.py:101-183 with the PeriodConv of
 * periodGATconv.py:204-236) with EVERYTHING that belongs to a destination node in one kernel: replaces the
 * destination-side columns of ggnn_project_batch (u_h, u4, S), ggnn_period_gat_aggregate_batch and
 * ggnn_lstm_epilogue_batch(GGNN_MODE_LSTM) -- same sums up to fp32 re-association.  Only the source-side value
 * rows V (one ggnn_project_batch with the value rows alone) go through memory; the score operands, the
 * aggregates and the gates' pre-activations never leave the compute unit.
 *
 * A workgroup of eight waves owns 128 consecutive destination nodes, one 16-node tile per wave, and walks the
 * gates in the order i, c~, f, o (the LSTM update is folded in as the gates arrive).  Per gate g and incoming
 * edge type e a wave (P1) multiplies its tile's [h | x | 1] rows with the (e, g) score weights -> u_h | u4 of its
 * 16 nodes, (P2) sweeps the tile's in-edges of that edge type (gathers of h_src and V rows, periodic min-image
 * correction, online-max softmax, relu, alpha-weighted sum: exactly ggnn_period_gat_aggregate_batch's arithmetic),
 * (P3) multiplies the 16 x 98 aggregate block with lin_l2 | (b_l2, w_edge) of (e, g) into the gate's
 * pre-activation, then (P4) adds the summed skip term of the gate.  Arithmetic of the three GEMMs: every fp32
 * operand as TWO fp16 pieces, hi = rne16(x) and lo' = rne16((x - hi) * 2048), and three of the four products
 * (hi hi + (hi lo' + lo' hi) / 2048) accumulated in fp32 on v_mfma_f32_16x16x32_f16: 22 significand bits per
 * operand, against an fp64 product 5e-8 of sum |x||w| (a plain fp32 fma chain: 2e-7); the rank-1 columns
 * (b_l2, w_edge) run on one exact fp32 MFMA.  The weights arrive as k-step slices of host-side pre-split planes
 * through a double-buffered LDS region shared by the eight waves (LDS-DMA).
 * OPERAND RANGE of the two-piece arithmetic: finite and |x| < 65504 for the weights, the tile's [h | x] rows and the
 * aggregates; the residual of an operand below 2^-13 in magnitude is subnormal (absolute resolution 2^-36).  A
 * weight outside the range cannot be packed (packing.split2_f16 refuses; packing.pack_cell then leaves the fused
 * operands out and the cell runs on projection + sweeps + gate GEMM, whose bf16 x 3 split covers fp32's range); an
 * activation outside it is clamped to +-65504 AND reported: the kernel ORs GGNN_FLAG_F16_RANGE into *flags (when
 * given), which graingraphnn_amd's backend reads at the end of a rollout / on request (range_exceeded).
 * FINITE OPERANDS are assumed by the sweep (round 6): it folds a row's in-edges three at a time WITHOUT a branch, the
 * slots behind the row's last edge filled with the (clamped) gather of a neighbouring edge and weighted with an exact
 * zero -- bit-identical to skipping them while the gathered hidden / value rows are finite; a NaN or inf in ANOTHER row
 * of h_src / v_src can then reach this row one step earlier than message passing would carry it (0 x inf).  The
 * flag word reports non-finite operands either way.
 *
 * Per incoming edge type:
 *   rowptr, col : destination-grouped CSR of the edge type (ggnn_build_csr_batch)
 *   einfo       : edge records in CSR order (ggnn_edge_prepare)
 *   h_src       : [n_src, ldh_src] hidden state of the source node type
 *   v_src       : [n_src, ldv] projection of the source node type; columns v_off + g * 96 .. + 95 = the value
 *                 rows of gate g for this edge type (first three input columns zeroed, as for the sweep)
 *   edge_params : [4][GGNN_EDGE_PARAM_ROWS][96] = W_value[:, 0..2] per gate
 * per problem (one destination node type of one model):
 *   x_dst [n_dst, ldx], h_dst [n_dst, ldh] (the encoder's h), c_in [n_dst, 96]; h_out, c_out [n_dst, 96]
 *   wstream : the weight slices in the order the kernel consumes them (packing.decoder_cell_stream):
 *             for g in (i, c~, f, o): for e: 4 slices P1(e, g) | 3 slices P3(e, g); then 4 slices P4(g) -- with e running
 *             FORWARDS over the incoming edge types for the first and third gate and BACKWARDS for the second and fourth
 *             (a pass re-gathers the hidden rows and edge records the pass before it gathered while L2 still holds them).
 *             Every slice is GGNN_DC_SLICE_BYTES: [column tile nb][plane hi, lo'][64 lanes][8 fp16] -- the two
 *             fp16 pieces of a weight w are hi = rne16(w) and lo' = rne16((w - hi) * 2048) (finite, |w| < 65504) --
 *             lane l = 16 kq + m of (nb, plane) holds W[16 nb + m][32 ks + 8 kq .. + 7]; P1 has 7 column tiles
 *             (u_h 0..95 | u4 96..111), P3 / P4 six (the tail of their slice is unused).  The reduction index
 *             of P1 / P4 is [h 0..95 | x 0..f_dst-1 | 1 (bias) | 0 ..] padded to 128, of P3 the 96 aggregate channels.
 *             The kernel splits its own operands the same way (OPERAND RANGE above).
 *   w2_tail : [4][n_in][6][64] fp32: (b_l2, w_edge) of (g, e) as v_mfma_f32_16x16x4_f32 A fragments
 *             ([ct][l] = k < 2 ? tail[16 ct + (l & 15)][k = l >> 4] : 0)
 *   flags   : optional int32 device word, see OPERAND RANGE
 * Gates are indexed i, f, c, o (GGNN_MODE_LSTM's order) in wstream's g, w2_tail, edge_params and the V columns.
 * n_src * ld < 2^31 for every gathered operand; up to four problems per call. */
#define GGNN_PRECISION_BF16 1
#define GGNN_PRECISION_F16X2 2
#define GGNN_OUT_BLOCK_MAJOR 0x100 /* or-ed into ggnn_project_args.precision: see there */
#define GGNN_DC_SLICE_BYTES 14336 /* 7 column tiles x 2 planes x 1 KB */
#define GGNN_FLAG_F16_RANGE 1     /* an activation at or beyond +-65504 was clamped in a two-piece fp16 split */
typedef struct ggnn_dec_cell_sweep {
  const int32_t* rowptr;     /* [n_dst + 1] */
  const int32_t* col;        /* [E] source node of every edge, CSR order */
  const float* einfo;        /* [E + GGNN_UNIT_EDGES, GGNN_EINFO_ROW] */
  const float* h_src;        /* [n_src, ldh_src] */
  const float* v_src;        /* [n_src, ldv] */
  const float* edge_params;  /* [4][GGNN_EDGE_PARAM_ROWS][96] */
  int64_t E, n_src, ldh_src, ldv;
  int32_t v_off;         /* first of the four gates' 96 value columns inside a v_src row (a multiple of 96 when block-major) */
  int32_t v_block_major; /* 0 = v_src is [n_src, ldv]; 1 = v_src is GGNN_OUT_BLOCK_MAJOR: [blocks][n_src][96], the
                            four gates' blocks v_off / 96 .. + 3 (ldv is ignored) */
} ggnn_dec_cell_sweep;
typedef struct ggnn_dec_cell_args {
  ggnn_dec_cell_sweep in[2];
  const float* x_dst;    /* [n_dst, ldx] */
  const float* h_dst;    /* [n_dst, ldh] */
  const float* c_in;     /* [n_dst, 96] */
  float* h_out;          /* [n_dst, 96] */
  float* c_out;          /* [n_dst, 96] */
  const void* wstream;   /* [n_slices][GGNN_DC_SLICE_BYTES], n_slices = 4 * (7 n_in + 4) */
  const float* w2_tail;  /* [4][n_in][6][64] */
  int32_t* flags;        /* optional: range flag word */
  int64_t n_dst, ldx, ldh;
  int32_t n_in, f_dst;
} ggnn_dec_cell_args;
int ggnn_decoder_cell_batch(const ggnn_dec_cell_args* args, int n_problems, ggnn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Training path: C[b] = A[b] . W[b]^T (+ C_in[b]) for a TALL A and a SMALL W -- the gate GEMM of a cell
 * (z_g = agg_g W2_g^T), its input gradient (g_agg_g = g_z_g W2_g) and the hidden-state gradient
 * (g_h += gP Wp[:, h columns]) of graingraphnn_amd/training.py, which replaces torch.bmm / torch.addmm there.
 *   a        : element (b, m, k) at a + b * a_bstride + m * lda + k        (M rows, K % 32 == 0, lda % 4 == 0)
 *   w        : element (b, n, k) at w + b * w_bstride + n * w_nstride + k * w_kstride  (n_out <= 224, n_out % 16 == 0;
 *              either orientation of a stored matrix: a gradient uses the transpose of the forward's weight)
 *   c, c_in  : element (b, m, n) at c + b * c_bstride + m * ldc + n; c_in optional (may equal c)
 *   precision: 0 = fp32-equivalent (two fp16 pieces per operand, three MFMA products; |w| < 65504; the rows of `a` may be
 *              ANY finite fp32 values -- every row is scaled by a power of two taken from its largest magnitude before it
 *              is split and the accumulators carry the factor, so gradient rows of 1e-10 keep the resolution activations
 *              of 1 have; a row holding an inf or a NaN gives NaN outputs, as an fp32 product would);
 *              GGNN_PRECISION_BF16 = one bf16 product, fp32 accumulation (what torch.autocast(bfloat16) defines)
 *   workspace: ggnn_rowgemm_workspace_bytes(K, n_out, batch) bytes, 16-byte aligned: the weights as MFMA operand
 *              planes (they change with every optimizer step).  prepacked == 0: the call packs them itself (two launches:
 *              pack, product); prepacked != 0: `workspace` already holds the planes of exactly this (w, K, n_out, batch,
 *              precision) from ggnn_rowgemm_pack -- one launch packs the weights of up to GGNN_ROWGEMM_MAX_PACK products
 *              (a training step packs the five products of a cell at once), `w` is not read.  (Not for fp32 products
 *              with n_out > 128 and K > 128, which run as two passes over column halves.)
 * a, c, c_in 16-byte aligned.  The product keeps a wave's 16 x n_out output tile in registers; the weight planes stay in
 * LDS for the whole launch (K <= 128, or <= 256 with n_out = 96) or stream through it. */
typedef struct ggnn_rowgemm_args {
  const float* a;
  const float* w;
  float* c;
  const float* c_in;
  void* workspace;
  size_t workspace_bytes;
  int64_t M, lda, ldc, a_bstride, c_bstride, w_bstride, w_nstride, w_kstride;
  int32_t K, n_out, batch, precision;
  int32_t prepacked, reserved;
} ggnn_rowgemm_args;
#define GGNN_ROWGEMM_MAX_PACK 8
size_t ggnn_rowgemm_workspace_bytes(int32_t K, int32_t n_out, int32_t batch);
int ggnn_rowgemm_pack(const ggnn_rowgemm_args* args, int n_products, ggnn_stream_t stream); /* reads w, K, n_out, batch, precision, workspace */
int ggnn_rowgemm(const ggnn_rowgemm_args* args, ggnn_stream_t stream);
/* TWO long products (args[0], args[1]: the streamed form -- K / 32 beyond what stays in LDS --, batch == 1, prepacked
 * planes, the same precision and n_out rounded to the same instantiated width) side by side in one grid: a wave walks the whole
 * reduction of its 16 rows, so such a product is M / 128 workgroups -- the hidden-state gradients of a training cell's two node
 * types (79 and 157 workgroups at the 10k-grain graph) then take the time of the longer one.  Same results as two calls;
 * anything else is refused (GGNN_EINVAL: make two calls). */
int ggnn_rowgemm_pair(const ggnn_rowgemm_args* args, ggnn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Output heads.
 * Regressor (models.py:433-452): y_joint = tanh(W_j h_j + b_j); y_grain = W_g h_g + b_g;
 * grain_area = tanh(y_grain[:,0])/20 + x_grain[:,3]; y_grain[:,0] = tanh; y_grain[:,1] = relu.
 *   w : [2][2][96] (joint rows, then grain rows), b : [2][2].
 */
int ggnn_heads_regressor(const float* h_joint, int64_t n_joint, const float* h_grain,
                         int64_t n_grain, const float* x_grain, int64_t ldx_grain,
                         const float* w, const float* b, float* y_joint, float* y_grain,
                         float* grain_area, ggnn_stream_t stream);
/* ggnn_heads_regressor followed by ggnn_step_update (below) in ONE launch: the heads write y_joint / y_grain /
 * grain_area (grain_area from the area the forward saw), then the same thread applies Rmodel.update and the z
 * advance to its node.  For a rollout step in which nothing reads x after this point (GrainRollout's
 * two-stream plan orders it behind the classifier's last reader of x). */
int ggnn_heads_regressor_update(const float* h_joint, int64_t n_joint, const float* h_grain,
                                int64_t n_grain, float* x_joint, int64_t ldx_joint, float* x_grain,
                                int64_t ldx_grain, int f_grain, const float* w, const float* b,
                                float* y_joint, float* y_grain, float* grain_area, float dz, float zmax,
                                int32_t* flags, ggnn_stream_t stream);
/* Classifier (models.py:595-609): pair = [h_j[src] | h_j[dst] | edge_attr];
 * edge_event = lin2(pair); edge = tanh(lin1(pair)).  Computed as per-node partial dots
 * (node_tmp [n_joint, 8] scratch) + a per-edge combine in the original COO order.
 *   w_node : [6][96] = lin1.w[0,0:96], lin1.w[1,0:96], lin2.w[0,0:96], lin1.w[0,96:192], lin1.w[1,96:192], lin2.w[0,96:192]
 *   w_edge : [6]     = lin1.w[0,192], lin1.w[1,192], lin2.w[0,192], lin1.b[0], lin1.b[1], lin2.b[0]
 * An edge with an endpoint outside [0, n_joint) gets NaN in its own three outputs (edge_event[e], edge[e, 0:2]) and reads
 * nothing; outputs behind *E_dev are not written.  (ggnn_step_refresh does the same with edge_attr[e].)
 */
int ggnn_heads_classifier(const float* h_joint, int64_t n_joint, const int64_t* edge_index_jj, int64_t E,
                          const int64_t* E_dev /* NULL, or the number of edges read from device memory when the kernels run:
                                                  edge_index_jj is [2, *E_dev] then, E the capacity the launch is sized for
                                                  (see ggnn_prepare_edge.E_dev) */,
                          const float* edge_attr_jj, const float* w_node, const float* w_edge, float* node_tmp,
                          float* edge_event, float* edge, ggnn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Rollout-step glue on device.
 * ggnn_step_update = GrainNN_regressor.update, periodic branch (models.py:503-516) + the z
 * advance of test.py:401-402:  x_j[:, :2] += y_j/5; x_j[:, 6:8] = y_j; x_g[:, 3] += y_g0/20;
 * x_g[:, 4] = y_g1; x_g[:, f_grain-1] = y_g0; z (column 2 of both) += dz.  flags[1] is set
 * to (x_grain[0, 2] > zmax) after the advance.
 * ggnn_step_refresh = the clamp of test.py:405-407 (if flags[1]: z = zmax on every node)
 * + the edge-length refresh of test.py:562-575 for up to three edge types:
 * edge_attr[e] = || min-image(src_xy - dst_xy) ||_2 in the original COO order.
 */
int ggnn_step_update(float* x_joint, int64_t n_joint, int64_t ldx_joint, float* x_grain,
                     int64_t n_grain, int64_t ldx_grain, int f_grain, const float* y_joint,
                     const float* y_grain, float dz, float zmax, int32_t* flags,
                     ggnn_stream_t stream);
/* Grain-centre refresh: replaces traj.GNN_update -> graph.update()
 * (graph_trajectory.py:1010-1085, graph_datastruct.py:681-708) + the write-back of
 * test.py:556-559.  For every grain with >= 2 junctions (CSR row of the joint->grain edge type
 * from ggnn_build_csr_batch): junction xy, brought to the global frame ((x + domain_offset[j]) /
 * domain_factor when domain_factor > 1, test.py:474), are chained by min-image to the previous
 * junction, shifted by +1 in a coordinate where any of them is below -1e-12, and averaged;
 * x_grain[g, 0:2] = centre, or frac(centre * domain_factor) when domain_factor > 1.
 * fp32 (the reference's numpy scalars promote to fp64: differences are <= 1 ulp of fp32).
 * Runs between ggnn_step_update and ggnn_step_refresh so that the refreshed edge lengths see the
 * new centres. */
#define GGNN_BC_PERIODIC 0
#define GGNN_BC_NOFLUX 1
int ggnn_grain_centres(const int32_t* rowptr, const int32_t* col, const float* x_joint, int64_t n_joint, int64_t ldx_joint,
                       const float* domain_offset /* [n_joint, 2], or NULL (= 0) */, float domain_factor, float* x_grain,
                       int64_t n_grain, int64_t ldx_grain,
                       float* centres_before /* NULL, or [n_grain, 2] that receives x_grain[:, 0:2] as the call found them (what
                                                a topological event of this step must see: the speculative event loop keeps it
                                                per step instead of copying the columns out) */,
                       int boundary /* GGNN_BC_PERIODIC: as above.  GGNN_BC_NOFLUX: no min-image chaining of the junctions
                                       (graph_datastruct.py:689-692 runs periodic_move for the periodic BC only), and
                                       rowptr / col are the FULL joint->grain CSR, so that grain 0 gets its centre too */,
                       ggnn_stream_t stream);
/* Event detection for the host-side topology update (test.py:418, models.py:624-626):
 * flags[0] = number of grains with live_grain > 0 and grain_area < area_threshold,
 * flags[1] = number of junction-junction edges with src < dst and edge_event (a logit) >
 * logit_threshold.  flags: [2] int32 device words, [3] with a range_word (zeroed by the call). */
int ggnn_detect_events(const float* grain_area, const int32_t* live_grain, int64_t n_grain, float area_threshold,
                       const float* edge_event, const int64_t* edge_index_jj, int64_t E,
                       const int64_t* E_dev /* NULL, or the number of junction edges read from device memory when the kernel
                                               runs: edge_index_jj is [2, *E_dev] then, E the capacity the launch is sized for
                                               (see ggnn_prepare_edge.E_dev) */,
                       float logit_threshold, int32_t* flags,
                       int32_t* range_word /* NULL, or an OPERAND RANGE word (ggnn_decoder_cell_batch) of the step whose
                                              predictions these are: flags[2] = the word's value, and the word is cleared for
                                              its next use (the speculative event loop reads a step's counts and its range
                                              report in one copy and drops the report of a step it voids: rollout.py) */,
                       int64_t skip_grain /* -1, or a grain that is never counted: the no-flux boundary grain, which
                                             test.py:421-422 drops from the candidates (its area feature is reset to 0 every
                                             step, so it is always below the threshold).  live_grain is not touched: the
                                             topology session reads the same mask */,
                       ggnn_stream_t stream);
/* ggnn_detect_events for a disjoint union of n_traj trajectories (one rollout of an ensemble): the same candidates, counted
 * per trajectory.  A grain belongs to the trajectory t with traj_grain_off[t] <= grain < traj_grain_off[t + 1], a junction
 * edge to the trajectory of its source junction (traj_joint_off); the offsets rise from 0 to the node counts, trajectories
 * may have any sizes.  counts [n_traj, 2] int32 = (grain candidates, switch candidates) of every trajectory whose `ended` word
 * is 0; flags[0:2] = their totals over those trajectories, flags[2] the range word as above.  counts and flags are zeroed by
 * the call (in one memset when counts directly follows the flag words).  Integer atomics only: exact, order-free. */
int ggnn_detect_events_traj(const float* grain_area, const int32_t* live_grain, int64_t n_grain, float area_threshold,
                            const float* edge_event, const int64_t* edge_index_jj, int64_t E, const int64_t* E_dev,
                            float logit_threshold, const int64_t* traj_grain_off /* [n_traj + 1], device */,
                            const int64_t* traj_joint_off /* [n_traj + 1], device */, int64_t n_traj,
                            const int32_t* ended /* NULL, or [n_traj] device words: non-zero = the trajectory takes part in
                                                    no events any more, its candidates are not counted */,
                            int64_t skip_local_grain /* must be -1.  A no-flux union keeps its boundary grains (every
                                                        trajectory's local grain 0) out of the count through live_grain: it
                                                        passes a candidate mask, the live mask with those grains' words at 0
                                                        (the live mask itself keeps 1 there: the QoI and the topology
                                                        sessions read it) */,
                            int32_t* counts, int32_t* flags, int32_t* range_word, ggnn_stream_t stream);
/* --- No-flux boundary (test.py:446-466, graph_datastruct.py:689-708 with traj.BC == 'noflux') ---
 * Grain 0 is the boundary grain that wraps the domain.
 * ggnn_noflux_boundary = the boundary step of test.py:446-463, one launch, after the topology update and before the
 * grain centres:  x_grain[0, 0:2] = 0.5, x_grain[0, 3:5] = 0, x_grain[0, f_grain-1] = 0; every junction to the global
 * frame, xy = (xy + domain_offset[j]) / domain_factor; every junction of grain 0's row of the FULL joint->grain CSR
 * (rowptr_jg / col_jg from ggnn_build_csr_batch) snapped to the nearest wall, argmin(x, 1-x, y, max_y-y), first minimum
 * wins (move_to_boundary, test.py:58-71); every junction clamped to [0,1] x [0,max_y]; back, xy = xy * domain_factor -
 * domain_offset[j].  fp32, each operation rounded on its own in the reference's order (no contraction).  domain_offset:
 * [n_joint, 2] or NULL (= 0).  joints_before: NULL, or [n_joint, 2] that receives x_joint[:, 0:2] as the call found
 * them (the speculative event loop's snapshot: a topological event of the step must see the junctions before it). */
int ggnn_noflux_boundary(const int32_t* rowptr_jg, const int32_t* col_jg, float* x_joint, int64_t n_joint,
                         int64_t ldx_joint, const float* domain_offset, float domain_factor, float max_y,
                         float* x_grain, int64_t ldx_grain, int f_grain, float* joints_before, ggnn_stream_t stream);
/* The boundary step for a disjoint union of n_traj trajectories, one launch of the same kernel: trajectory t owns the
 * junctions [traj_joint_off[t], traj_joint_off[t + 1]) and the grains from traj_grain_off[t] on, its boundary grain is its
 * first one, g0 = traj_grain_off[t].  Per trajectory with junctions: row g0 of x_grain reset as above, the junctions of row
 * g0 of the FULL joint->grain CSR snapped to the nearest wall; every junction of the union clamped.  domain_factor, max_y:
 * one box for the whole union; domain_offset: [n_joint, 2], the trajectories' concatenated.  The offsets ([n_traj + 1] int64,
 * device) rise from 0 to the node counts; a trajectory with junctions must own at least one grain (equal offsets: an empty
 * trajectory, skipped).  ggnn_noflux_boundary is the case of one trajectory. */
int ggnn_noflux_boundary_traj(const int32_t* rowptr_jg, const int32_t* col_jg, float* x_joint, int64_t n_joint,
                              int64_t ldx_joint, const float* domain_offset, float domain_factor, float max_y,
                              float* x_grain, int64_t ldx_grain, int f_grain, float* joints_before,
                              const int64_t* traj_grain_off, const int64_t* traj_joint_off, int64_t n_traj,
                              ggnn_stream_t stream);
/* --- Process parameters on the device (the reference's --temporal mode, test.py:345-346, 376-379) ---
 * ggnn_process_schedule = the thermal gradient and pulling speed features of the step to come, one launch at the tail of a
 * step, in front of the launch that builds the next step's edge records.  For every junction j of trajectory t
 *   x_joint[j, 3] = table[r, t, 0],  x_joint[j, 4] = table[r, t, 1],  r = min(max(*step_in + 1, 0), n_rows - 1),
 * and the launch leaves *step_in + 1 in *step_out (INT32_MAX stays): row r belongs to the r-th step from a counter of 0, a
 * captured graph replays with the counter where the replay before left it, past the last row the last row holds, and the
 * table is never addressed outside [0, n_rows) for any counter value.
 * table: [n_rows, n_traj, 2] fp32, device: FEATURE values (1 - G / 10 and R / 2, rounded to fp32 once by the host from
 * float64: the reference's assignment of a float64 scalar into a float32 tensor).  The kernel only copies: bit for bit.
 * traj_joint_off: [n_traj + 1] int64, device, rising from 0 to n_joint; trajectories may have any size or be empty; a
 * junction belongs to the last trajectory whose offset is <= the junction.  NULL: one trajectory (n_traj must be 1).
 * Nothing but columns 3 and 4 of rows [0, n_joint) is written (no padding column of ldx_joint > the feature count).
 * step_in / step_out: int32 device words, the same word or different ones (the speculative event loop keeps one per ring
 * slot): every block reads the counter before the last block to finish stores it.  sync_word: one zeroed int32 device
 * word, left zero by every launch; not shared by launches that may run concurrently.  The results do not depend on the
 * grid.  GGNN_EINVAL: a NULL required pointer, n_joint < 1, n_rows < 1, n_traj < 1, ldx_joint < 5, NULL offsets with
 * n_traj != 1. */
int ggnn_process_schedule(float* x_joint, int64_t n_joint, int64_t ldx_joint, const float* table, int64_t n_rows,
                          int64_t n_traj, const int64_t* traj_joint_off, const int32_t* step_in, int32_t* step_out,
                          int32_t* sync_word, ggnn_stream_t stream);
/* --- Quantities of interest of a rollout (graph_trajectory.py:1042-1051 GNN_update "qoi", :221-242 volume('graph'),
 * :244-256 qoi) ---
 * Per trajectory t = grains [traj_offsets[t], traj_offsets[t+1]) of a disjoint-union graph, with F = domain_factor,
 * s = patch_size / mesh_size + 1, live = live_grain > 0 (NULL: every grain):
 *   A_k    = sum_g live * x_grain[g, 3] / F^2
 *   a_k[g] = live ? x_grain[g, 3] * s^2 / A_k : 0        (a trajectory without a live grain: all zeros, no division)
 *   e_k[g] = live ? x_grain[g, 4] / 20 * s^3 : 0
 *   T_k    = T_{k-1} + delta_h / 2 * (a_{k-1} + a_k)     (delta_h = span * (final_height - ini_height) / mesh_size / (frames - 1))
 *   volume_k = V0 + T_k + e_k
 * ggnn_qoi_accumulate = ONE layer, one launch, behind the step's topology update and boundary step.  The layer index is
 * k = *layer_in + 1, read from device memory when the kernel runs, and the launch leaves k in *layer_out: a captured
 * graph replays with the counter where the replay before left it.  layer_in / layer_out, a_prev / a_cur and T_in / T_out
 * may be the same buffers (every element is read and written by one thread; the counter is advanced by the last block to
 * finish, through sync_word) or different ones (the speculative event loop keeps one state per ring slot).
 * init != 0 = layer 0: k = 0, a_0 by the formula above or copied from area0 (the reference keeps the rasterised pixel
 * counts there, test.py:340), V0 = 4 / (3 sqrt(pi)) a_0^1.5 is WRITTEN, T_0 = 0, history row 0 = V0.
 * history: NULL, or [capacity + 1, n_grain]: row k = volume_k.  A layer k > capacity writes no row and ORs
 * GGNN_FLAG_QOI_OVERFLOW into *flags; a_cur / T_out / e_cur are still advanced.  Nothing outside the arrays is addressed
 * for any traj_offsets (entries are clamped to [0, n_grain]).
 * Arithmetic: fp64 per grain and in the sums, rounded to fp32 where stored.  A_k is a tree of fixed shape over the
 * trajectory's grains counted from its first one (no floating-point atomics): the results do not depend on the grid, on
 * the launch plan or on where the trajectory sits in a union, bit for bit.  Inputs must be finite.
 * sync_word: one zeroed int32 device word, left zero by every launch; not shared by launches that may run concurrently. */
#define GGNN_FLAG_QOI_OVERFLOW 2  /* ggnn_qoi_accumulate: a layer beyond the history's capacity */
typedef struct ggnn_qoi_args {
  const float* x_grain;         /* [n_grain, ldx_grain >= 5]: column 3 area, column 4 excess volume */
  const int32_t* live_grain;    /* [n_grain] or NULL */
  const int64_t* traj_offsets;  /* [n_traj + 1], device */
  const float* area0;           /* init only: NULL or [n_grain] */
  const float* a_prev;          /* [n_grain] a_{k-1} */
  const float* T_in;            /* [n_grain] T_{k-1} */
  float* V0;                    /* [n_grain]: read; written by init */
  float* a_cur;                 /* [n_grain] a_k */
  float* T_out;                 /* [n_grain] T_k */
  float* e_cur;                 /* [n_grain] e_k */
  float* history;               /* NULL or [capacity + 1, n_grain] */
  float* area_sum;              /* NULL or [n_traj]: A_k */
  const int32_t* layer_in;      /* k - 1 */
  int32_t* layer_out;           /* receives k */
  int32_t* sync_word;
  int32_t* flags;
  int64_t ldx_grain, n_grain, n_traj, capacity;
  double domain_factor, s, delta_h;
  int32_t init, reserved;
} ggnn_qoi_args;
int ggnn_qoi_accumulate(const ggnn_qoi_args* args, ggnn_stream_t stream);
/* ggnn_qoi_finalize: volume = V0 + T + e, size = cbrt(6 volume / pi) * mesh_size per grain, and per trajectory over ALL of
 * its grains (eliminated ones included, as np.mean / np.std there): d_mu, d_std (population; two passes: the mean, then
 * the squared deviations from it, fp64 trees of fixed shape) and hist [n_traj, n_edges - 1] = the counts of np.histogram
 * for bin_edges ([n_edges] ascending fp32, device; half-open bins, the last one closed; sizes are compared as fp32).
 * n_edges = 0: no histogram; at most 1025 edges. */
int ggnn_qoi_finalize(const float* V0, const float* T, const float* e, int64_t n_grain, const int64_t* traj_offsets,
                      int64_t n_traj, double mesh_size, const float* bin_edges, int n_edges, float* volume, float* size,
                      float* d_mu, float* d_std, int32_t* hist, ggnn_stream_t stream);
/* --- The grains' junction polygons of a rollout layer (graph.update(), graph_datastruct.py:654-721: `regions`,
 * `region_coors`, `region_center`) ---
 * ggnn_grain_polygons = ONE layer, one launch, behind the step's topology update, boundary step and centre refresh; it only
 * reads the state.  Per grain g with row [p0, p1) of the joint->grain table (rowptr / col: the table ggnn_grain_centres reads,
 * the FULL one for GGNN_BC_NOFLUX; read from device memory when the kernel runs, so a captured graph follows the events
 * that rewrite the table in place; entries are clamped, nothing outside [0, E_cap) and [0, n_joint) is addressed):
 *   unwrap : junction xy in the global frame ((x + domain_offset[j]) / domain_factor when domain_factor > 1); periodic: each
 *            junction min-imaged to the previous moved one in the row's order (no-flux: no chaining); then +1 in a
 *            coordinate where any vertex of the row is below -1e-12.  Exactly ggnn_grain_centres' coordinates.
 *   centre : (the sum of the unwrapped coordinates in the row's order) / n, +1 where the vertices were shifted.  Unfolded:
 *            frac(centre * domain_factor) belongs to x_grain, not to the polygon.
 *   order  : ascending in the key of counterclock() (:100-116) -- the angle of d = v - centre in [0, 2 pi), then |d|, then
 *            the position in the row.  The kernel compares (quadrant, q, |dx| + |dy|, position) with quadrant 0..3 counted
 *            from dx > 0, dy >= 0 (d = 0: quadrant -1, first) and q = |dy| / (|dx| + |dy|) in quadrants 0 and 2, |dx| /
 *            (|dx| + |dy|) in 1 and 3: the same order as the angle's wherever two angles differ by more than a few ulp, the
 *            same 0 / 2 pi seam (the sign of dy), and only additions, comparisons and one correctly rounded division.
 *            GGNN_BC_NOFLUX: the boundary grain's order is reversed (:715-716) -- grain 0, or with traj_grain_off the first
 *            grain of every trajectory that has grains.
 *   area   : half the sum of cross(d_i, d_next(i)) over the ordered polygon (negative for a reversed one).
 * All of it in fp32, every operation that decides the order rounded on its own in one fixed sequence: the results do not
 * depend on the grid or on the row's path through the kernel, bit for bit (the area's sum is a tree of fixed shape).
 * A row of 0 or 1 junction is copied as it is, with area 0 and the centre at the junction (0 for an empty row).
 * Outputs are rows of per-layer arrays in the table's own layout (sides of g = rowptr_out[g + 1] - rowptr_out[g]); layer
 * k = *layer_in + 1 (NULL: k = 0) is read from device memory when the kernel runs and left in *layer_out (NULL: no counter),
 * the same word or another one, advanced by the last block to finish through sync_word (one zeroed int32 device word,
 * left zero, not shared by launches that may run concurrently).  A layer outside [0, capacity] writes nothing and ORs
 * GGNN_FLAG_POLYGON_OVERFLOW into *flags.  Elements of joint_sorted / xy_sorted behind rowptr[n_grain] are not written.
 * GGNN_EINVAL: a NULL required pointer, no such boundary, n_joint / n_grain < 1, ldx_joint < 2, E_cap or capacity outside
 * [0, INT32_MAX), domain_factor < 1, traj_grain_off with n_traj < 1 (without: n_traj != 1), layer_out without sync_word /
 * flags. */
#define GGNN_FLAG_POLYGON_OVERFLOW 4  /* ggnn_grain_polygons: a layer beyond the arena's capacity */
typedef struct ggnn_polygon_args {
  const int32_t* rowptr;           /* [n_grain + 1] */
  const int32_t* col;              /* [E_cap] junction of every table entry */
  const float* x_joint;            /* [n_joint, ldx_joint >= 2] */
  const float* domain_offset;      /* NULL (= 0) or [n_joint, 2] */
  const int64_t* traj_grain_off;   /* NULL or [n_traj + 1], device: the trajectories' first grains (GGNN_BC_NOFLUX) */
  int32_t* rowptr_out;             /* [capacity + 1, n_grain + 1]: row k = a copy of rowptr */
  int32_t* joint_sorted;           /* [capacity + 1, E_cap] */
  float* xy_sorted;                /* [capacity + 1, E_cap, 2] */
  float* centre;                   /* [capacity + 1, n_grain, 2] */
  float* area;                     /* [capacity + 1, n_grain] */
  const int32_t* layer_in;         /* NULL (layer 0) or k - 1 */
  int32_t* layer_out;              /* NULL or receives k */
  int32_t* sync_word;
  int32_t* flags;
  int64_t n_joint, ldx_joint, n_grain, E_cap, n_traj, capacity;
  float domain_factor;
  int32_t boundary;                /* GGNN_BC_PERIODIC / GGNN_BC_NOFLUX */
} ggnn_polygon_args;
int ggnn_grain_polygons(const ggnn_polygon_args* args, ggnn_stream_t stream);
/* ggnn_polygon_inputs = what a layer's ggnn_grain_polygons launch reads, kept beside its record so that two layers can be
 * blended afterwards (ggnn_interp_polygons): one launch IN FRONT of that launch, on the same stream, writes row
 * k = *layer_in + 1 (NULL: k = 0) -- the word the polygon launch reads; this launch does not advance it -- of
 *   col_out  [capacity + 1, E_cap]      : col[0 .. E_cap) as it is (the polygon launch clamps what it reads, so do the readers),
 *   joint_xy [capacity + 1, n_joint, 2] : the junctions in the global frame, the expression ggnn_grain_polygons unwraps from
 *                                         ((x + domain_offset[j]) / domain_factor when domain_factor > 1).
 * A layer outside [0, capacity] writes nothing (the polygon launch raises GGNN_FLAG_POLYGON_OVERFLOW).  Plain loads and
 * stores.  GGNN_EINVAL: a NULL col / x_joint / col_out / joint_xy, n_joint < 1, ldx_joint < 2, E_cap or capacity outside
 * [0, INT32_MAX), domain_factor < 1. */
typedef struct ggnn_polygon_inputs_args {
  const int32_t* col;              /* [>= E_cap] */
  const float* x_joint;            /* [n_joint, ldx_joint >= 2] */
  const float* domain_offset;      /* NULL (= 0) or [n_joint, 2] */
  int32_t* col_out;                /* [capacity + 1, E_cap] */
  float* joint_xy;                 /* [capacity + 1, n_joint, 2] */
  const int32_t* layer_in;         /* NULL (layer 0) or k - 1 */
  int64_t n_joint, ldx_joint, E_cap, capacity;
  float domain_factor;
} ggnn_polygon_inputs_args;
int ggnn_polygon_inputs(const ggnn_polygon_inputs_args* args, ggnn_stream_t stream);
/* --- In-between layers of a rollout (test.py:494-528, --interp_frames) ---
 * ggnn_interp_polygons = n_jobs <= GGNN_INTERP_MAX_JOBS polygon records blended from recorded layers, the job a grid
 * dimension; on demand, on `stream`; it only reads the recorder's arrays (rowptr of ggnn_grain_polygons, col_out / joint_xy
 * of ggnn_polygon_inputs).  Job i = (layer L = job_layer[i] in [1, layers], coefficient c = job_coeff[i] in [0, 1]), HOST
 * arrays; row i of the outputs -- the layout of ggnn_grain_polygons' five arrays with capacity + 1 = n_jobs, which
 * ggnn_polygons_rasterize reads unchanged.  The rule (tests/interpcheck.py restates it), all of it in fp32, every operation
 * rounded on its own:
 *   topology : layer T = L where c > 0.5 (compared in double), else L - 1 (test.py:502-514); the job's rowptr and col are
 *              layer T's recorded ones, O is the other layer of the two.
 *   seam     : GGNN_BC_PERIODIC: per junction and coordinate layer O's value is brought to the minimum image of layer T's:
 *              o += rel > 0.5 ? -1 : (rel < -0.5 ? 1 : 0) with rel = o - t.
 *   blend    : v = fl(fl(c) * X_L) + fl(fl(1 - c) * X_{L-1}); 1 - c is formed in double and rounded once.
 *   wrap     : GGNN_BC_PERIODIC: v -= floorf(v) where v is not in [0, 1) although layer T's coordinate is.  (Recorded
 *              junctions are never wrapped and a few lie below 0; next to such a coordinate v stays where the blend put it,
 *              so that the endpoints below hold for every recorded layer.)
 *   no-flux  : GGNN_BC_NOFLUX, move_to_boundary and the clamps (test.py:58-70, 502-508): every junction of the boundary
 *              grain's row of layer T's table (grain 0, or with traj_grain_off the first grain of every trajectory that has
 *              grains) takes d = {x, 1 - x, y, max_y - y} of the UNCLAMPED blend, the FIRST minimum decides, and that
 *              coordinate becomes 0, 1, 0 or max_y; every other coordinate of every junction is clamped to [0, 1] x
 *              [0, max_y].  The positions are finished per junction in `work` before any row reads them, so a snapped
 *              junction is seen snapped by every grain that holds it.  Periodic jobs neither snap nor clamp (there grain 0
 *              is an ordinary grain).
 *   rows     : ggnn_grain_polygons' rule on those positions with layer T's table, domain_factor 1: the same device code.
 * (L, 1.0) reproduces layer L's record and (L, 0.0) layer L - 1's (joint_sorted, xy_sorted as numbers, centre): always
 * (periodic), wherever the recorded junctions lie inside the box with the boundary grain's on the walls, as the step's
 * boundary launch leaves them (no-flux).
 * Launches: blend (one thread per junction and job), GGNN_BC_NOFLUX: snap (one block per trajectory and job; it forms the
 * blend of its junctions again and overwrites the snapped coordinate), rows -- two or three, whatever n_jobs is.
 * Table entries and layers are clamped: nothing outside the arrays is addressed, whatever they hold.
 * GGNN_EINVAL without a launch: args or a pointer other than traj_grain_off NULL, no such boundary, n_joint / n_grain < 1,
 * E_cap or capacity outside [0, INT32_MAX), layers outside [1, capacity], n_jobs outside [1, GGNN_INTERP_MAX_JOBS], a job with
 * a layer outside [1, layers] or c outside [0, 1] (NaN included), GGNN_BC_NOFLUX without max_y > 0, traj_grain_off with
 * n_traj < 1 (without: n_traj != 1). */
#define GGNN_INTERP_MAX_JOBS 256
typedef struct ggnn_interp_args {
  const int32_t* rowptr;           /* [capacity + 1, n_grain + 1], device: the recorder's */
  const int32_t* col;              /* [capacity + 1, E_cap], device: ggnn_polygon_inputs' col_out */
  const float* joint_xy;           /* [capacity + 1, n_joint, 2], device: ggnn_polygon_inputs' */
  const int64_t* traj_grain_off;   /* NULL or [n_traj + 1], device (GGNN_BC_NOFLUX) */
  const int32_t* job_layer;        /* HOST [n_jobs] */
  const double* job_coeff;         /* HOST [n_jobs] */
  float* work;                     /* [n_jobs, n_joint, 2], device: the finished positions */
  int32_t* rowptr_out;             /* [n_jobs, n_grain + 1] */
  int32_t* joint_sorted;           /* [n_jobs, E_cap] */
  float* xy_sorted;                /* [n_jobs, E_cap, 2] */
  float* centre;                   /* [n_jobs, n_grain, 2] */
  float* area;                     /* [n_jobs, n_grain] */
  int64_t n_joint, n_grain, E_cap, capacity, layers, n_traj, n_jobs;
  float max_y;
  int32_t boundary;                /* GGNN_BC_PERIODIC / GGNN_BC_NOFLUX */
} ggnn_interp_args;
int ggnn_interp_polygons(const ggnn_interp_args* args, ggnn_stream_t stream);
/* --- The grain-ID image of recorded layers (plot_polygons, graph_datastruct.py:553-610: `alpha_field`) ---
 * ggnn_polygons_rasterize = n_layers rows of ggnn_grain_polygons' arena filled into image [n_layers, ny, nx] int32 (periodic:
 * [n_layers, nx, nx]), indexed [y][x]; the call zeroes the image itself, then ONE launch takes up to GGNN_RASTER_MAX_LAYERS
 * layers (the layer is a grid dimension; more layers: one launch per such group).  On demand, on `stream`; it only reads
 * the arena.  The rule is exact in integers (tests/rastercheck.py restates it):
 *   vertices   : of polygon row [rowptr[g], rowptr[g + 1]) of xy_sorted, with s = nx for BOTH coordinates:
 *                GGNN_BC_PERIODIC v = (int)(x * (float)s) -- one fp32 product, truncated toward zero; GGNN_BC_NOFLUX
 *                v = (int)rintf(x * (float)s) -- half to even.  The product saturates at +-2^20 (NaN: -2^20).
 *   membership : a lattice point belongs to a polygon when it lies on one of its edges, or has an odd number of crossings
 *                under the half-open rule in y (edge a -> b with ya < yb counts on ya <= y < yb for points strictly left of
 *                it): the closed set of the even-odd rule, decided by the sign of (x - xa)(yb - ya) - (y - ya)(xb - xa) in
 *                int64.  The kernel takes it from the edge's crossing with the scanline, xc = xa + num / den with
 *                num = (y - ya)(xb - xa), den = yb - ya > 0, rounded both ways: with q = num / den truncated toward zero
 *                and r = num - q den, floor = q - (r < 0) and ceil = q + (r > 0) -- a negative numerator truncates
 *                upward, so there the floor is corrected and the ceiling is not; x < xc <=> x < ceil, x = xc <=> ceil <=
 *                x <= floor.  Rows of 0 or 1 junction draw nothing; a row of 2 draws the lattice points of its segment.
 *   ownership  : image = max(grain index - grain_begin + 1) over the polygons that hold the point; 0 = uncovered.  A max:
 *                the image does not depend on the grid or on the order of arrival.
 *   periodic   : canvas [0, 2 nx)^2, points outside dropped, folded by mod nx with max (the four quadrants' np.max).
 *   no-flux    : canvas [0, nx) x [0, ny), points outside dropped; the boundary grain is skipped (grain 0, or with
 *                traj_grain_off the first grain of every trajectory that has grains); with_corners: an uncovered pixel takes
 *                corner_grains[2 x / nx + 2 (2 y / ny)] (:602-605), otherwise it stays 0.
 * Only grains [grain_begin, grain_end) are drawn (a trajectory of a union).  Table entries are clamped: nothing outside the
 * arena rows and the image is addressed, whatever the tables hold.
 * GGNN_EINVAL without a launch: args / rowptr / xy_sorted / image NULL, no such boundary, nx or ny outside [1, 2^15), n_grain
 * < 1, E_cap or capacity outside [0, INT32_MAX), a grain range outside [0, n_grain], traj_grain_off with n_traj < 1 (without:
 * n_traj != 1), n_layers < 1, a layer outside [0, capacity]. */
#define GGNN_RASTER_MAX_LAYERS 256
typedef struct ggnn_raster_args {
  const int32_t* rowptr;           /* [capacity + 1, n_grain + 1], device: the arena's */
  const float* xy_sorted;          /* [capacity + 1, E_cap, 2], device: the arena's */
  const int64_t* traj_grain_off;   /* NULL or [n_traj + 1], device (GGNN_BC_NOFLUX) */
  const int32_t* layers;           /* HOST [n_layers]: the arena rows to draw, or NULL: rows 0 .. n_layers - 1 */
  int32_t* image;                  /* [n_layers, ny, nx] (periodic: [n_layers, nx, nx]), device */
  int64_t n_grain, E_cap, capacity, n_traj, grain_begin, grain_end, n_layers, nx, ny;
  int32_t corner_grains[4];
  int32_t with_corners;
  int32_t boundary;                /* GGNN_BC_PERIODIC / GGNN_BC_NOFLUX */
} ggnn_raster_args;
int ggnn_polygons_rasterize(const ggnn_raster_args* args, ggnn_stream_t stream);
/* ggnn_image_compare = one launch over n_pixels int32 pixels: *differing += the pixels where image != truth (truth and
 * differing both NULL: not compared), counts[id] += the pixels with that id for 0 <= id <= n_grain (counts NULL: not counted;
 * other ids are not counted).  Both accumulate on what the caller left there, with 64-bit integer atomics: exact, and
 * independent of the order.  GGNN_EINVAL without a launch: image NULL, n_pixels < 1, n_grain outside [0, INT32_MAX), truth
 * without differing or the reverse, neither truth nor counts. */
int ggnn_image_compare(const int32_t* image, const int32_t* truth, int64_t n_pixels, int64_t n_grain, uint64_t* differing,
                       uint64_t* counts, ggnn_stream_t stream);
/* ------------------------------------------------------------------------------------
 * The junction graph of a grain-ID image: the inverse of ggnn_polygons_rasterize, the way into a rollout for a structure
 * that exists as an image (an EBSD map, a phase-field cross-section).  The reference has no such step: its graphs come from
 * its generator or from its phase-field solver's junction tracks (`node_region`, graph_trajectory.py:316-376).  On demand,
 * on `stream`; setup work, not part of a step.  Periodic images and images with no-flux walls (`boundary`, below); a stack
 * of equal-shaped images -- the trajectories of a union, or the frames of a sequence, each on its own -- goes through the
 * _traj forms further down; the frames of a sequence are matched to one another by ggnn_track_junctions below.  Stacks of
 * mixed shapes and resolving a quadruple from a history are not covered.
 * ggnn_image_junctions = memset of the status + three launches (count per block, scan of the blocks, emit).  The rule is
 * exact in integers up to the one fp32 expression of a position (tests/vectorcheck.py restates it):
 *   image     : int32 [ny, nx], pixel p = grain p - 1 (as ggnn_polygons_rasterize writes), periodic in both directions
 *   window    : (y, x) = the pixels TL (y, x), TR (y, x + 1), BL (y + 1, x), BR (y + 1, x + 1), indices mod ny / nx; its
 *               raster index is y nx + x
 *   keys      : a window with a pixel outside [1, n_grain] carries none; with three distinct ids it carries that sorted
 *               triple; with four (a quadruple) the two triples {TL, TR, BR} and {TL, BL, BR} -- the TL-BR diagonal,
 *               always, and counted; otherwise none.  Every pixel outside [1, n_grain] is counted once.
 *   junctions : a window is the REPRESENTATIVE of a key it carries when no window of a smaller raster index at an offset
 *               |dy|, |dx| <= merge_radius (the periodic minimum image; nx, ny > 2 merge_radius) carries the same key.
 *               Every (representative, key) is one junction; junctions are numbered in raster order of the window and,
 *               within a window, by ascending key.  A carried key that is not represented counts as merged.  The
 *               numbering does not depend on the grid.
 *   position  : with m = the windows at such offsets that carry the key, the representative (yr, xr) included, and
 *               (Sx, Sy) = the sums of their offsets: x = ((float)xr + offset + (float)Sx / (float)m) * pitch, each
 *               operation rounded to fp32 on its own in this order -- the quotient, (float)xr + offset, their sum, the
 *               product; y likewise from yr and Sy.  offset = 1, pitch = 1 / nx restates the rasteriser's convention
 *               (s = nx); offset = 0.5, pitch = 1 / (nx - 1) suits samples on a grid that includes both ends.  Positions
 *               are not wrapped into [0, 1).
 *   columns   : junction j with the 0-based grains g0 < g1 < g2: triples[j] = (g0, g1, g2); columns 3j .. 3j + 2 of the
 *               grain->joint list edge_gj [2, 3 joint_capacity] (row 1 at edge_gj + 3 joint_capacity) = (g_k, j)
 *   status    : int64 [GGNN_JUNCTION_STATUS_WORDS], zeroed by the call: n_joint, n_quad_windows, n_merged_windows,
 *               n_invalid_pixels, n_open_pairs (ggnn_junction_links), n_present_grains (ids g with pixel_counts[g] != 0,
 *               1 <= g <= n_grain), overflow (n_joint > joint_capacity).  Nothing is written at or beyond joint_capacity,
 *               and nothing between n_joint and it.  The structure is VALID when overflow, n_invalid_pixels and
 *               n_open_pairs are 0 and n_joint == 2 n_present_grains (Euler's formula on the torus).
 * boundary = GGNN_BC_NOFLUX: the image has walls, and everything outside it is grain 0, the boundary grain that wraps the
 * domain (its row of the joint->grain table holds every wall junction, as in the reference's no-flux graphs, where a junction
 * lies on a wall exactly when its triple holds grain 0 and two wall junctions are linked exactly when they share (0, a)).
 * The rule above with these changes (tests/vectorcheck_noflux.py restates it):
 *   image     : not periodic.  Valid ids inside are [2, n_grain]: a pixel that is 1 or outside [1, n_grain] is counted in
 *               n_invalid_pixels and voids its windows.
 *   window    : (y, x) for y in [-1, ny - 1], x in [-1, nx - 1]; a pixel outside the image reads as id 1 (resolved in
 *               registers: no padded copy of the image is made); raster index (y + 1)(nx + 1) + (x + 1).
 *   keys      : as above.  A window on a wall holds two outside pixels and a corner window three, so neither holds four
 *               ids, and a corner window {1, 1, 1, a} carries nothing: corners are not junctions in the reference, they
 *               are its corner_grains.
 *   junctions : as above with offsets (y' - y, x' - x) clipped by the window range, not wrapped; nx, ny > 2 merge_radius.
 *   position  : the same expression (xr, yr may be -1); then for a junction whose triple holds grain 0 -- its
 *               representative straddles a wall, since only such windows read an outside pixel -- the coordinate normal to
 *               that wall is set exactly: xr == -1: x = 0.0f, xr == nx - 1: x = 1.0f, yr == -1: y = 0.0f, yr == ny - 1:
 *               y = max_y = ((float)(ny - 2) + 2 offset) / ((float)(nx - 2) + 2 offset), each operation rounded to fp32
 *               (ny / nx for offset 1, (ny - 1) / (nx - 1) for offset 0.5, exactly 1 for a square image); the coordinate no
 *               wall has set is clamped to [0, 1] (x) or [0, max_y] (y), which acts next to a corner only, where the
 *               carriers of one key lie on two walls.  Every junction then lies in [0, 1] x [0, max_y] with grain 0's on the
 *               walls, so ggnn_noflux_boundary(max_y) leaves the positions as they are.
 *   status    : n_present_grains counts the ids 2 .. n_grain; VALID: overflow, n_invalid_pixels and n_open_pairs 0 and
 *               n_joint == 2 n_present_grains - 2 (Euler's formula on the sphere, grain 0 being the outer face).
 * The grid is ny + 1 rows of ceil((nx + 1) / GGNN_JUNCTION_SEGMENT) segments, and the workspace holds one word a block.
 * GGNN_EINVAL without a launch: args or a pointer NULL, status / edge_gj / pixel_counts not 8-byte aligned, merge_radius
 * outside [0, 7], nx or ny outside (2 merge_radius, 2^15), n_grain outside [1, INT32_MAX - 1), joint_capacity outside
 * [1, INT32_MAX / 3], offset outside [0, 1], pitch outside (0, 1], boundary neither GGNN_BC_PERIODIC nor GGNN_BC_NOFLUX, a
 * workspace below ny ceil(nx / GGNN_JUNCTION_SEGMENT) words (periodic) or (ny + 1) ceil((nx + 1) / GGNN_JUNCTION_SEGMENT)
 * words (no-flux).
 * ggnn_junction_links = one launch: column 3j + k of the joint->joint list edge_jj [2, 3 joint_capacity] = (j, partner) for
 * the pairs (g0, g1), (g0, g2), (g1, g2) of junction j < min(n_joint, joint_capacity) in that order; the partner is the one
 * OTHER junction below that bound whose triple holds both grains, found by walking the first grain's row of the
 * joint->grain table (ggnn_build_csr_batch on the flipped edge_gj: no sort, no hash); -1 when there is none or more than
 * one, and the slot is counted in status[4] (zeroed by the call; it reads status[0]).  Rows and columns are clamped to
 * [0, E_cap] and [0, n_joint).  GGNN_EINVAL without a launch: args or a pointer NULL, status / edge_jj not 8-byte aligned,
 * n_grain or joint_capacity as above, E_cap outside [0, INT32_MAX). */
#define GGNN_JUNCTION_SEGMENT 256
#define GGNN_JUNCTION_STATUS_WORDS 7
typedef struct ggnn_junction_args {
  const int32_t* image;          /* [ny, nx], device */
  const uint64_t* pixel_counts;  /* [n_grain + 1], device: ggnn_image_compare's counts of the image */
  float* xy;                     /* [joint_capacity, 2] out */
  int32_t* triples;              /* [joint_capacity, 3] out */
  int64_t* edge_gj;              /* [2, 3 joint_capacity] out */
  int64_t* status;               /* [GGNN_JUNCTION_STATUS_WORDS] out */
  int32_t* workspace;            /* ny * ceil(nx / GGNN_JUNCTION_SEGMENT) int32 words of device scratch (no-flux: see above) */
  size_t workspace_bytes;
  int64_t nx, ny, n_grain, joint_capacity;
  float offset, pitch;
  int32_t merge_radius;
  int32_t boundary;              /* GGNN_BC_PERIODIC / GGNN_BC_NOFLUX */
} ggnn_junction_args;
int ggnn_image_junctions(const ggnn_junction_args* args, ggnn_stream_t stream);
typedef struct ggnn_link_args {
  const int32_t* triples;        /* [joint_capacity, 3], device: ggnn_image_junctions' */
  const int32_t* rowptr;         /* [>= n_grain + 1]: the joint->grain table's row pointers */
  const int32_t* col;            /* [E_cap]: its columns */
  int64_t* edge_jj;              /* [2, 3 joint_capacity] out */
  int64_t* status;               /* ggnn_image_junctions' status: word 0 is read, word 4 written */
  int64_t n_grain, joint_capacity, E_cap;
} ggnn_link_args;
int ggnn_junction_links(const ggnn_link_args* args, ggnn_stream_t stream);
/* The same for a STACK of images, into the disjoint union of their graphs: images int32 [n_image, ny, nx] (one shape a
 * stack), image b holding the union's grains grain_off[b] .. grain_off[b + 1] - 1, pixel p of image b = union grain
 * grain_off[b] + p - 1.  The rule is the one above applied per image, for both boundaries: windows, keys, the TL-BR diagonal,
 * representatives within merge_radius, the fp32 position expression in its order, the wall snap and max_y -- with n_grain =
 * grain_off[b + 1] - grain_off[b], read on the device.  A periodic wrap, a clipped no-flux offset and a no-flux outside pixel
 * stay inside their image; indices into the stack are 64-bit.
 *   numbering : junctions image after image, raster order (then ascending key) within an image: the blocks are laid out
 *               image-major, (image, row, segment), so block order is union order and one scan block serves, as above.
 *               triples and row 0 of edge_gj hold UNION grains, row 1 of edge_gj and both rows of edge_jj union junctions.
 *   status    : int64 [n_image, GGNN_JUNCTION_STATUS_WORDS], zeroed by the call: the seven words above per image --
 *               n_present_grains counts that image's ids, n_invalid_pixels judges a pixel by its own image's grain count,
 *               n_open_pairs goes to the image of the junction, overflow is 1 for every image whose last junction lies
 *               beyond joint_capacity (the capacity is the union's) -- and DIRECTLY BEHIND them joint_off int64
 *               [n_image + 1], written by the scan: image b's junctions are joint_off[b] .. joint_off[b + 1] - 1 and
 *               joint_off[n_image] is the union's n_joint (not clamped to the capacity).  One read-back fetches both.
 *   counts    : pixel_counts uint64 [n_grain] (n_grain = the union's), zeroed and filled by the count pass: the pixels of
 *               union grain g = the pixels of its image with the id g - grain_off[b] + 1, exact; ids outside the image's range
 *               are not counted.  No launch per image, and none beside the three.
 *   grain_off : device memory, so not validated but clamped: every offset to [0, n_grain], an image's end to its begin at
 *               least.  An image with no grain carries nothing: all its pixels are invalid.
 * Nothing is written at or beyond joint_capacity, and nothing between the union's n_joint and it.  The launches -- two
 * memsets, count, scan, emit -- do not depend on n_image.  The grid is n_image * rows * segments blocks (rows and segments as
 * above for the boundary), at most GGNN_JUNCTION_MAX_BLOCKS: a block holds at most 512 junctions, so the int32 scan cannot
 * overflow.  GGNN_EINVAL without a launch: as ggnn_image_junctions (n_grain is the union's; grain_off too must be 8-byte
 * aligned), n_image < 1, a grid beyond GGNN_JUNCTION_MAX_BLOCKS, a workspace below one word a block.
 * ggnn_junction_links_traj = two launches: word 4 of every status row zeroed, then ggnn_junction_links' search on the union
 * (rowptr / col: the union's joint->grain table; a pair's partner lies in its first grain's row and so in its own image);
 * an open slot is counted in the row of the image that joint_off puts its junction in.  It reads joint_off behind the status
 * rows.  GGNN_EINVAL without a launch: as ggnn_junction_links, and n_image outside [1, GGNN_JUNCTION_MAX_BLOCKS]. */
#define GGNN_JUNCTION_MAX_BLOCKS (1 << 22)
typedef struct ggnn_junction_traj_args {
  const int32_t* images;         /* [n_image, ny, nx], device */
  const int64_t* grain_off;      /* [n_image + 1], device, rising from 0 */
  uint64_t* pixel_counts;        /* [n_grain] out */
  float* xy;                     /* [joint_capacity, 2] out */
  int32_t* triples;              /* [joint_capacity, 3] out */
  int64_t* edge_gj;              /* [2, 3 joint_capacity] out */
  int64_t* status;               /* [n_image * GGNN_JUNCTION_STATUS_WORDS + n_image + 1] out: the status rows, then joint_off */
  int32_t* workspace;            /* one int32 word a block of device scratch */
  size_t workspace_bytes;
  int64_t nx, ny, n_image, n_grain, joint_capacity;   /* n_grain, joint_capacity: the union's */
  float offset, pitch;
  int32_t merge_radius;
  int32_t boundary;              /* GGNN_BC_PERIODIC / GGNN_BC_NOFLUX */
} ggnn_junction_traj_args;
int ggnn_image_junctions_traj(const ggnn_junction_traj_args* args, ggnn_stream_t stream);
typedef struct ggnn_link_traj_args {
  const int32_t* triples;        /* [joint_capacity, 3], device: ggnn_image_junctions_traj's */
  const int32_t* rowptr;         /* [>= n_grain + 1]: the union's joint->grain table's row pointers */
  const int32_t* col;            /* [E_cap]: its columns */
  int64_t* edge_jj;              /* [2, 3 joint_capacity] out */
  int64_t* status;               /* ggnn_image_junctions_traj's: joint_off is read, word 4 of every row written */
  int64_t n_grain, joint_capacity, E_cap, n_image;
} ggnn_link_traj_args;
int ggnn_junction_links_traj(const ggnn_link_traj_args* args, ggnn_stream_t stream);
/* Linking by TRACING BOUNDARIES: a second linking rule for the columns the rule above leaves open because MORE than one other
 * junction holds the pair -- two grains that share two separate stretches of boundary: a lens on a boundary one frame before
 * it vanishes, a band that reaches from wall to wall.  Such a structure is legal (three-fold junctions, Euler's formula holds);
 * the boundary in the image says which two junctions each stretch joins.  Per image of a union, both boundaries, exact in
 * integers; tests/tracecheck.py restates the rule.  A structure without open pairs is left as it is, bit for bit.
 * ggnn_image_junction_windows_traj = ggnn_image_junctions_traj -- the same checks, launches and results -- with one more
 * output: rep int32 [joint_capacity], rep[j] = the raster index of junction j's representative window within its image (y nx +
 * x, no-flux (y + 1)(nx + 1) + (x + 1)); nothing at or beyond joint_capacity or n_joint.  GGNN_EINVAL also for rep NULL.
 * ggnn_junction_links_trace_traj, after ggnn_junction_links_traj = a memset of its counters + one launch, a thread a
 * joint->joint column of a junction j < min(n_joint, joint_capacity); a column that is not -1 returns at once.
 *   vertex    : a window (y, x) of the junction rule, with its range, its periodic wrap and its outside-reads-as-id-1 convention
 *   cracks    : of a vertex: UP between TL and TR to (y - 1, x), DOWN between BL and BR to (y + 1, x), LEFT between TL and BL to
 *               (y, x - 1), RIGHT between TR and BR to (y, x + 1); an a | b crack has the ids of grains a and b as its two pixels
 *   owner     : a window W that carries key k is owned by the junction of smallest index (below the bound above, in W's image)
 *               that has triple k and whose representative lies at an offset within merge_radius of W -- wrapped for periodic,
 *               plain for no-flux --, found by walking the joint->grain row of the key's last grain and comparing triple and
 *               rep (no sort, no hash).  A carrier that no junction owns belongs to nobody (carriers that chain-merge).
 *   owned by j: the windows at offsets within merge_radius of rep[j] that carry j's triple and whose owner for it is j
 *   exits     : for j and its pair (a, b): the a | b cracks from a vertex owned by j to a vertex not owned by j
 *   diagonals : for j and (a, b): the quadruple windows owned by j whose TL and BR are a and b
 *   walk      : j has no diagonal and exactly one exit: follow it.  At every vertex reached: if the window carries a key that
 *               holds both a and b, stop -- its owner is o.  Otherwise the vertex must have exactly two a | b cracks, the one
 *               arrived by and one more: leave by the other.  The walk FAILS at a vertex with another number of them (four is
 *               the two-id checkerboard window [a b; b a]) and at a carrier nobody owns; it OVERFLOWS when more than max_trace
 *               vertices would be reached.
 *   accept    : partner(j, pair) = o only if o too has no diagonal and exactly one exit for (a, b) (worked out by the same
 *               thread): that exit is the crack arrived by, so the thread of o's column reaches j by the reversed walk of the
 *               same length -- the result is symmetric, and a thread writes its own column only.
 *   quadruple : j has exactly one diagonal W for (a, b): o = the owner of W's other key, and partner(j, pair) = o when o too has
 *               exactly one diagonal for (a, b) and it is W.  There is no crack to follow.  Several diagonals fail.
 *   counters  : int64 [n_image, GGNN_TRACE_COUNTERS], zeroed by the call: n_traced, n_trace_failed (no exit or several, a failed
 *               walk, a refused partner), n_trace_overflow -- directed columns, counted at the image of the junction; every open
 *               column is counted in exactly one.  Status word 4 (n_open_pairs) of the image loses one per traced column and so
 *               becomes what is still open: the validity tests read it unchanged.  Integer sums; no result is ordered by one,
 *               so a replay gives the same bits.
 * Pixel reads wrap or clip inside their image with 64-bit indices; nothing is read or written at or beyond joint_capacity; rows
 * and columns of the table are clamped as in ggnn_junction_links, grain offsets as above, a rep outside its image's windows
 * owns nothing; (2 merge_radius + 1)^2, E_cap and max_trace bound every loop.  GGNN_EINVAL without a launch: args or a pointer
 * NULL, a 64-bit array not 8-byte aligned or a 32-bit one not 4-byte aligned, n_grain, joint_capacity, E_cap, n_image as in
 * ggnn_junction_links_traj, nx, ny, merge_radius, boundary as in ggnn_image_junctions_traj, max_trace < 1.
 * Not covered: matching the two junctions of a lens between frames (they share a triple: ggnn_track_junctions counts them as
 * ambiguous and leaves them unmatched), structures that fail Euler's formula (a grain with a part that is not even
 * corner-connected to its body; a neck through a pixel corner is read by GGNN_PINCH_NECK below). */
#define GGNN_TRACE_COUNTERS 3
int ggnn_image_junction_windows_traj(const ggnn_junction_traj_args* args, int32_t* rep, ggnn_stream_t stream);
typedef struct ggnn_link_trace_args {
  const int32_t* images;         /* [n_image, ny, nx], device: ggnn_image_junction_windows_traj's */
  const int64_t* grain_off;      /* [n_image + 1], device */
  const int32_t* triples;        /* [joint_capacity, 3] */
  const int32_t* rep;            /* [joint_capacity]: ggnn_image_junction_windows_traj's */
  const int32_t* rowptr;         /* [>= n_grain + 1]: the union's joint->grain table's row pointers */
  const int32_t* col;            /* [E_cap]: its columns */
  int64_t* edge_jj;              /* [2, 3 joint_capacity]: ggnn_junction_links_traj's; the open columns of row 1 are written */
  int64_t* status;               /* the status rows, then joint_off: joint_off is read, word 4 of the rows updated */
  int64_t* counters;             /* [n_image, GGNN_TRACE_COUNTERS] out */
  int64_t nx, ny, n_image, n_grain, joint_capacity, E_cap;
  int64_t max_trace;             /* the vertices a walk may reach, at least 1 (the Python layer's default: 4 (nx + ny)) */
  int32_t merge_radius;
  int32_t boundary;              /* GGNN_BC_PERIODIC / GGNN_BC_NOFLUX */
} ggnn_link_trace_args;
int ggnn_junction_links_trace_traj(const ggnn_link_trace_args* args, ggnn_stream_t stream);
/* PINCH WINDOWS: a second reading of one window pattern, beside the junction rule above and a mode of the same kernels.  A
 * pinch window is a window of three distinct valid ids whose repeated id sits on a diagonal: [a b; c a] (TL == BR) or
 * [b a; a c] (TR == BL).  The junction rule gives it the key {a, b, c}: a junction where grains b and c meet.  They do not
 * meet: grain a runs through the corner as a neck one pixel wide, and the a | b boundary and the a | c boundary each turn
 * through the vertex.  (The other reading, b touching c, would cut grain a in two, which the graph cannot hold either.)  A
 * grain-ID image whose cell edges drift below a pixel shows such windows, and each is one junction too many for Euler's formula.
 *   GGNN_PINCH_JUNCTION : the rule above, its kernels, launch for launch and bit for bit.
 *   GGNN_PINCH_NECK     : a window of three distinct valid ids CARRIES NO KEY when TL == BR or TR == BL.  Valid ids, the
 *                         periodic wrap and the no-flux outside-reads-as-id-1 convention are unchanged, and so are quadruple
 *                         windows and the two-id checkerboard [a b; b a].  "Carries" is the one predicate every part of the
 *                         rule reads, so a pinch window is no candidate; it is no carrier in the representative test of another
 *                         window; it is not in m, Sx, Sy of a junction's position; it is not counted as merged; in the trace rule
 *                         it owns nothing and nobody owns it, and a walk that reaches it finds a vertex with exactly two a | b
 *                         cracks and leaves by the other, as the walk rule above says of any vertex without a key.
 *   n_pinch_windows     : int64 [n_image], zeroed by the call (one memset more): under GGNN_PINCH_NECK the pinch windows of every
 *                         image, each counted once, an integer sum of the count pass (one atomic a wave, as n_quad_windows; no
 *                         result is ordered by it); under GGNN_PINCH_JUNCTION the call is the plain one and the words stay 0.
 *                         The status row keeps its GGNN_JUNCTION_STATUS_WORDS words; the counters may lie in the caller's
 *                         status buffer behind everything else, so that one read-back fetches them too.
 * The _pinch_traj entry points are their namesakes with the mode (the single-image entry points have no twin: an image is the
 * union of one).  ggnn_junction_links_trace_pinch_traj takes the mode the images were vectorised with and no counters: it counts
 * nothing new.  GGNN_EINVAL without a launch: as their namesakes, a mode that is neither of the two, n_pinch_windows NULL or not
 * 8-byte aligned.  tests/pinchcheck.py restates the rule. */
#define GGNN_PINCH_JUNCTION 0
#define GGNN_PINCH_NECK 1
int ggnn_image_junctions_pinch_traj(const ggnn_junction_traj_args* args, int32_t pinch, int64_t* n_pinch_windows,
                                    ggnn_stream_t stream);
int ggnn_image_junction_windows_pinch_traj(const ggnn_junction_traj_args* args, int32_t* rep, int32_t pinch,
                                           int64_t* n_pinch_windows, ggnn_stream_t stream);
int ggnn_junction_links_trace_pinch_traj(const ggnn_link_trace_args* args, int32_t pinch, ggnn_stream_t stream);
/* ------------------------------------------------------------------------------------
 * Training targets from a recorded SEQUENCE of grain-ID images: the n_frame images of one union above are the frames of a
 * sequence in which a grain keeps its id (local grain g of every frame is the same grain; an eliminated grain no longer
 * occurs), and the two calls derive from the union's arrays what the reference's junction tracker (graph_trajectory.py:283-846)
 * and GrainHeterograph.form_gradient (graph_datastruct.py:851-1011) derive from its phase-field solver's output.  Setup work,
 * on `stream`, nothing through the host; tests/trackcheck.py restates the rule.
 *   frames    : frame t is VALID when its status row is (overflow, n_invalid_pixels, n_open_pairs 0 and Euler's formula for
 *               `boundary`), judged on the device; the PAIR (t, t + 1) is emitted when both frames are valid.
 *   match     : a junction's LOCAL triple is its triple minus its frame's grain_off.  Junction j of frame t matches junction
 *               k of frame t + 1 when the pair is emitted, their local triples are equal and that triple occurs exactly once
 *               in frame t and exactly once in frame t + 1: next_joint[j] = k, prev_joint[k] = j (union indices), otherwise
 *               -1.  A junction of frame t whose triple occurs more than once in frame t or in frame t + 1 is AMBIGUOUS.
 * ggnn_track_junctions = a memset of its counters + one launch, a thread a junction j < min(n_joint, joint_capacity): it walks
 * the joint->grain row of the triple's first grain in its own, the next and the previous frame and counts equal triples.
 * counters int64 [n_frame, 2], zeroed by the call: n_matched, n_ambiguous of the pair (t, t + 1), counted at frame t.
 * ggnn_track_targets = a memset of its counters + two launches (a thread a joint->joint column; a thread a union grain):
 *   y_joint   : matched j -> k: fp32(5.0 * d), d = (double)xy[k] - (double)xy[j] per coordinate, for GGNN_BC_PERIODIC the
 *               minimum image (d > 0.5: d - 1; d < -0.5: d + 1); mask_joint = 1.  Unmatched: y 0, mask 0.
 *   hist_joint: the same expression from prev_joint[j] to j (x_joint columns 6, 7 of the reference), 0 without one.
 *   edge_label: per column s = 3 j + k of edge_jj, u = j, v its destination, in a frame whose pair is emitted: 0 when u and
 *               v are both matched and next_joint[u], next_joint[v] are linked in frame t + 1 (one is the destination of a
 *               column of the other); 1 (a neighbour switch) when both are unmatched and, with u = {a, b, c}, v = {a, b, d},
 *               the triples {a, c, d} and {b, c, d} each occur exactly once in frame t + 1 and those two junctions are linked;
 *               -1 (unlabelled) otherwise, and for every column of a frame whose pair is not emitted.
 *   y_grain   : with c, c' the pixel counts of the grain in frames t, t + 1: [0] = fp32(20.0 * ((double)c' / patch_pixels -
 *               (double)c / patch_pixels)), [1] = fp32(20.0 * extra_volume[grain in t + 1]) (0 when extra_volume is NULL);
 *               mask_grain = 1 where c != 0 (never for local grain 0 of GGNN_BC_NOFLUX, the boundary grain); grain_event = 1
 *               where the mask is 1 and c' == 0.  All 0 in a frame whose pair is not emitted.
 *   hist_grain: [0] = the area expression from frame t - 1 to t when the pair (t - 1, t) is emitted, else 0 (x_grain column
 *               10); [1] = fp32(20.0 * extra_volume[grain]) (x_grain column 4); both 0 for a grain without pixels in frame t
 *               and for a no-flux boundary grain.
 *   counters  : int64 [n_frame, 4], zeroed by the call: the directed columns labelled 0, 1, -1 and the grain events of the
 *               pair (t, t + 1), counted at frame t (frames without an emitted pair count nothing).
 * The counters are integer atomics (sums); no result is ordered by one, so a replay gives the same bits.  Nothing is read or
 * written at or beyond joint_capacity, rows and columns of the table are clamped as in ggnn_junction_links, grain offsets to
 * [0, n_grain].  GGNN_EINVAL without a launch: args or a pointer NULL (extra_volume may be), a 64-bit array not 8-byte
 * aligned, n_grain, joint_capacity, E_cap as in ggnn_junction_links, n_frame outside [2, GGNN_JUNCTION_MAX_BLOCKS], boundary
 * neither GGNN_BC_PERIODIC nor GGNN_BC_NOFLUX, patch_pixels below 1. */
typedef struct ggnn_track_args {
  const int32_t* triples;        /* [joint_capacity, 3], device: ggnn_image_junctions_traj's */
  const int32_t* rowptr;         /* [>= n_grain + 1]: the union's joint->grain table's row pointers */
  const int32_t* col;            /* [E_cap]: its columns */
  const int64_t* grain_off;      /* [n_frame + 1], device */
  const int64_t* status;         /* [n_frame * GGNN_JUNCTION_STATUS_WORDS + n_frame + 1]: the status rows, then joint_off */
  int64_t* next_joint;           /* [joint_capacity] out */
  int64_t* prev_joint;           /* [joint_capacity] out */
  int64_t* counters;             /* [n_frame, 2] out */
  int64_t n_grain, joint_capacity, E_cap, n_frame;
  int32_t boundary;              /* GGNN_BC_PERIODIC / GGNN_BC_NOFLUX */
  int32_t reserved;
} ggnn_track_args;
int ggnn_track_junctions(const ggnn_track_args* args, ggnn_stream_t stream);
typedef struct ggnn_track_targets_args {
  const int32_t* triples;        /* as above */
  const int32_t* rowptr;
  const int32_t* col;
  const int64_t* edge_jj;        /* [2, 3 joint_capacity]: ggnn_junction_links_traj's */
  const float* xy;               /* [joint_capacity, 2] */
  const uint64_t* pixel_counts;  /* [n_grain] */
  const double* extra_volume;    /* [n_grain] in union order, or NULL */
  const int64_t* grain_off;
  const int64_t* status;
  const int64_t* next_joint;     /* ggnn_track_junctions' */
  const int64_t* prev_joint;
  float* y_joint;                /* [joint_capacity, 2] out */
  float* mask_joint;             /* [joint_capacity] out */
  float* hist_joint;             /* [joint_capacity, 2] out */
  int64_t* edge_label;           /* [3 joint_capacity] out */
  float* y_grain;                /* [n_grain, 2] out */
  float* mask_grain;             /* [n_grain] out */
  int64_t* grain_event;          /* [n_grain] out */
  float* hist_grain;             /* [n_grain, 2] out */
  int64_t* counters;             /* [n_frame, 4] out */
  double patch_pixels;
  int64_t n_grain, joint_capacity, E_cap, n_frame;
  int32_t boundary;
  int32_t reserved;
} ggnn_track_targets_args;
int ggnn_track_targets(const ggnn_track_targets_args* args, ggnn_stream_t stream);
/* ------------------------------------------------------------------------------------
 * The way in from a MEASURED map: an orientation map (an EBSD scan: angles per pixel, non-indexed points, speckle) or a noisy
 * id image becomes the grain-ID image and the per-grain angles that the calls above take.  Setup work, on `stream`, nothing
 * through the host, exact in integers; tests/labelcheck.py restates the rule.  One image a call (T images a call:
 * ggnn_label_grains_stack, after ggnn_label_orientations).
 *   input     : one image [ny, nx], nx, ny >= 3, `boundary` GGNN_BC_PERIODIC or GGNN_BC_NOFLUX, in one of two forms.
 *               ids: int32; a pixel is VALID when id >= 1 and the optional byte mask `valid` is non-zero there; two
 *               4-neighbours are LINKED when both are valid and their ids are equal.
 *               angles: float32 [K, ny, nx], 1 <= K <= 4 (the model's case: K = 2, theta_x and theta_z in radians); a pixel
 *               is valid when every channel is finite with |a| <= 8 and the mask allows it; two 4-neighbours are linked when
 *               both are valid and fabsf(a_k - b_k) <= tol for every k -- one fp32 subtraction a channel, symmetric by IEEE.
 *               Linking is not transitive in the angle: it is the usual pixel-to-pixel misorientation criterion.
 *               Neighbours wrap under GGNN_BC_PERIODIC and do not exist beyond a wall under GGNN_BC_NOFLUX.  The raster
 *               index of a pixel is y nx + x.
 *   components: the classes of the valid pixels under the links.  A component's ROOT is its smallest raster index, its size
 *               its pixel count.
 *   cleanup   : a component of fewer than min_pixels pixels is a SPECK (min_pixels >= 1; 1: no valid pixel is cleaned up).
 *               Speck pixels and invalid pixels are OPEN, all others CLOSED, carrying their root.  Jacobi sweeps: sweep s
 *               reads the state after sweep s - 1; every open pixel collects the roots of the closed ones among its four
 *               neighbour positions (left, right, up, down, by the boundary rule above); if there is any it takes the root
 *               that occurs most often among them, a tie going to the smaller root, and is closed from the next sweep on.
 *               The sweeps end after max_sweeps, or after one that assigned nothing.  Pixels still open are UNFILLED and are
 *               written 0 (ggnn_image_junctions counts them in n_invalid_pixels).  Components grow and never merge, so
 *               roots are stable.
 *   numbering : the components closed before the first sweep are the grains, ranked by ascending root.  Periodic: pixel =
 *               rank + 1, n_grain = their number.  No-flux: pixel = rank + 2, n_grain = their number + 1: grain 0 (id 1) is
 *               the boundary grain and does not occur inside, as ggnn_image_junctions requires.
 *   means     : (K > 0) per grain and channel over the pixels of the ORIGINAL component (absorbed pixels carry noise and do
 *               not count): q = __float2ll_rn(__fmul_rn(a, 16777216.0f)), S = the int64 sum of q, n = the original size,
 *               mean = (float)((double)S / (double)n / 16777216.0).  |a| <= 8 and fewer than 2^30 pixels: S fits 2^57, the
 *               sum is exact and independent of the order.  mean_angles is [K, grain_capacity], row g of channel k at
 *               k grain_capacity + g; no-flux: row 0 is 0.  Rows from n_grain on are not written.
 *   status    : int64 [GGNN_LABEL_STATUS_WORDS], zeroed by the call: n_components (before the cleanup), n_specks,
 *               n_speck_pixels, n_invalid_in, n_grains (the closed components: n_grain without the boundary grain),
 *               n_sweeps (sweeps that assigned something), n_unfilled, overflow (n_grain > grain_capacity: the image is
 *               still complete, the per-grain rows hold the first grain_capacity grains), n_bound_hits (must be 0: a
 *               thread that followed parents beyond the bound derived from the image size counted itself and left).
 * ggnn_label_grains = two memsets and 9 + 2 max_sweeps launches, whatever the image holds: links (a byte a pixel), tiles (a
 * workgroup a GGNN_LABEL_TILE_X x GGNN_LABEL_TILE_Y tile: union-find on labels in LDS, tile-local roots, counts and angle sums),
 * seams (linked pairs across tile edges and the wrap: atomicMin on the larger root's parent, retried from the new roots),
 * flatten, classify (closed / open, the list of open pixels, the counters), per sweep decide + commit (a sweep after one that
 * assigned nothing returns on a device word), the rank as block sums, scan of the sums and add (with the means), the image.
 * No kernel waits on another workgroup; every loop over parents is bounded.  Nothing outside the image, the workspace, the
 * status and grain_capacity rows of mean_angles is addressed, whatever the inputs hold.
 * GGNN_EINVAL without a launch: args, image, status or workspace NULL, both or neither of ids / angles, nx or ny outside
 * [3, 2^15), with angles K outside [1, 4], mean_angles NULL or tol not >= 0, with ids K != 0, min_pixels < 1, max_sweeps
 * outside [0, GGNN_LABEL_MAX_SWEEPS], grain_capacity outside [1, INT32_MAX), an unknown boundary, status or workspace not
 * 8-byte aligned, a 32-bit array not 4-byte aligned, a workspace below ggnn_label_workspace_bytes(nx, ny, K) (which is 0 for
 * sizes the call refuses).
 * A stack of equal-shaped maps in the same launches is ggnn_label_grains_stack below (ggnn_link_labels then gives a sequence's
 * grains ids that persist across the frames).  Not covered: 8-connectivity.  The per-channel rule knows no crystal symmetry (a grain that
 * straddles the wrap of an angle comes out as two): full orientations under cubic symmetry are ggnn_label_orientations below. */
#define GGNN_LABEL_TILE_X 64
#define GGNN_LABEL_TILE_Y 16
#define GGNN_LABEL_STATUS_WORDS 9
#define GGNN_LABEL_MAX_SWEEPS 1024
typedef struct ggnn_label_args {
  const int32_t* ids;            /* [ny, nx], device, or NULL */
  const float* angles;           /* [K, ny, nx], device, or NULL: exactly one of the two */
  const uint8_t* valid;          /* [ny, nx] bytes, device, or NULL: every pixel allowed */
  int32_t* image;                /* [ny, nx] out */
  float* mean_angles;            /* [K, grain_capacity] out (NULL with ids) */
  int64_t* status;               /* [GGNN_LABEL_STATUS_WORDS] out */
  void* workspace;               /* ggnn_label_workspace_bytes(nx, ny, K) of device scratch */
  size_t workspace_bytes;
  int64_t nx, ny, grain_capacity, min_pixels;
  float tol;
  int32_t K;                     /* channels of angles; 0 with ids */
  int32_t max_sweeps;
  int32_t boundary;              /* GGNN_BC_PERIODIC / GGNN_BC_NOFLUX */
} ggnn_label_args;
size_t ggnn_label_workspace_bytes(int64_t nx, int64_t ny, int32_t K);
int ggnn_label_grains(const ggnn_label_args* args, ggnn_stream_t stream);
/* ------------------------------------------------------------------------------------
 * The same segmentation for FULL ORIENTATIONS under crystal symmetry (an EBSD map: a Bunge triple a pixel, which the indexing
 * software reports as any of the 24 cubic equivalents, changing from pixel to pixel inside one grain).  Only the link decision
 * and the per-grain mean differ from ggnn_label_grains; tests/orientcheck.py restates both.  Every fp32 and fp64 operation
 * below is rounded on its own (__fmul_rn, __fadd_rn, __fsub_rn, __dmul_rn, __dadd_rn, __ddiv_rn, __dsqrt_rn, no contraction),
 * in the order written, so that a float32 / float64 restatement gives the same bits.
 *   input     : quats float32 [4, ny, nx] (planes w, x, y, z; component k of pixel p at k ny nx + p): the unit quaternion that
 *               takes crystal to sample coordinates; q and -q are the same orientation.  nx, ny in [3, 2^15).  A pixel is
 *               VALID when the optional byte mask `valid` allows it and fabsf(n - 1) <= 1e-3f with n = ((w w + x x) + y y) + z z
 *               (a NaN or an inf in any component fails the comparison).
 *   product   : p (x) q, the one evaluation every product below uses, each component four fp32 products combined left to right:
 *                 w = ((pw qw - px qx) - py qy) - pz qz        x = ((pw qx + px qw) + py qz) - pz qy
 *                 y = ((pw qy - px qz) + py qw) + pz qx        z = ((pw qz + px qy) - py qx) + pz qw
 *               conj(q) = (w, -x, -y, -z).
 *   link      : two valid 4-neighbours a (the pixel) and b (its right or lower neighbour, by the boundary rule of
 *               ggnn_label_grains) are LINKED when W >= cos_half_tol, where r = conj(q_a) (x) q_b, m1 >= m2 >= m3 >= m4 are
 *               |r_w|, |r_x|, |r_y|, |r_z| sorted, h = GGNN_ORIENT_H and
 *                 GGNN_SYM_CUBIC: W = max(m1, (m1 + m2) h, 0.5 ((m1 + m2) + (m3 + m4)))
 *                 GGNN_SYM_NONE : W = |r_w|.
 *               The cubic form is the largest |w(r (x) s)| over the 24 proper cubic rotations s, i.e. cos of half the
 *               DISORIENTATION angle; swapping a and b negates r_x, r_y, r_z exactly, so the link is symmetric.
 *               cos_half_tol = (float)cos((double)tol / 2) is formed by the caller, 0 < tol < pi/2, tol the largest
 *               disorientation in radians that still links.  fp32 resolves W to 6e-8, which is about 1e-5 rad of tol at tol =
 *               1 degree and coarser below (tol < 4.9e-4 rad gives cos_half_tol = 1).
 *   then      : components, cleanup, numbering and the nine status words are ggnn_label_grains', word for word.
 *   operators : s_0 .. s_23 (w, x, y, z), h = GGNN_ORIENT_H = 0.70710678f; GGNN_SYM_NONE uses s_0 alone:
 *                 s_0 = (1, 0, 0, 0)       s_1 = (0, 1, 0, 0)       s_2 = (0, 0, 1, 0)       s_3 = (0, 0, 0, 1)
 *                 s_4 = (h, h, 0, 0)       s_5 = (h, -h, 0, 0)      s_6 = (h, 0, h, 0)       s_7 = (h, 0, -h, 0)
 *                 s_8 = (h, 0, 0, h)       s_9 = (h, 0, 0, -h)      s_10 = (0, h, h, 0)      s_11 = (0, h, -h, 0)
 *                 s_12 = (0, h, 0, h)      s_13 = (0, h, 0, -h)     s_14 = (0, 0, h, h)      s_15 = (0, 0, h, -h)
 *                 s_16 = (0.5, 0.5, 0.5, 0.5)       s_17 = (0.5, 0.5, 0.5, -0.5)     s_18 = (0.5, 0.5, -0.5, 0.5)
 *                 s_19 = (0.5, 0.5, -0.5, -0.5)     s_20 = (0.5, -0.5, 0.5, 0.5)     s_21 = (0.5, -0.5, 0.5, -0.5)
 *                 s_22 = (0.5, -0.5, -0.5, 0.5)     s_23 = (0.5, -0.5, -0.5, -0.5)
 *   means     : per grain over the pixels p of its ORIGINAL component with root rho: r = conj(q_rho) (x) q_p, c_i = the w
 *               component of r (x) s_i by the product above, i* = the first i with the largest |c_i|, a = q_p (x) s_i*,
 *               negated when c_i* < 0 (a zero counts as positive): the equivalent of q_p nearest the root's.  Q_k =
 *               __float2ll_rn(__fmul_rn(a_k, 16777216.0f)), S_k = the int64 sum of Q_k over the component: exact, whatever the
 *               order.  d_k = (double)S_k, n2 = ((d_0 d_0 + d_1 d_1) + d_2 d_2) + d_3 d_3, mean_k = (float)(d_k / sqrt(n2)), and
 *               q_rho itself when n2 == 0.  mean_quats is [4, grain_capacity], component k of grain g at k grain_capacity + g;
 *               no-flux: row 0 is (1, 0, 0, 0).  Rows from n_grain on are not written.  The mean is one of the 24 (48 with
 *               signs) equivalents, the one near the root pixel's.  A component whose pixels drift more than about 20 degrees
 *               from its root (links are not transitive) can align a pixel to the wrong equivalent: a property of the rule.
 * ggnn_label_orientations = two memsets and 12 + 2 max_sweeps launches, whatever the map holds: ggnn_label_grains' with its
 * links kernel replaced (a thread a pixel: its quaternion, the right and the lower neighbour's, two products, a four-element
 * sorting network, the same byte a pixel) and three added: after classify the sums are zeroed at the roots and every closed
 * pixel is aligned to its root and accumulated (a wave sums runs of consecutive pixels with one root by shuffles, in 32 bits,
 * and the head of a run issues the four 64-bit integer atomics: no result depends on an order); after the rank the means are
 * normalised and written.  The three rules of ggnn_label_grains hold: no kernel waits on another workgroup, every walk over
 * parents is bounded and counted in n_bound_hits, nothing outside quats, valid, image, status, the workspace and
 * grain_capacity rows of mean_quats is addressed.
 * Measured on one MI355X: 4 096 x 4 096 with 2 048 cells and 1 % noise, min_pixels 8: 2 300 us a call against 2 158
 * us for ggnn_label_grains on two angle channels of the same cells; links 95 us (17 bytes a pixel, 2.7 x its traffic floor),
 * zero 14 us, accumulate 342 us (8.2 x its floor: the 24 products a pixel), means 20 us.  501 x 501: 481 against 465 us.
 * GGNN_EINVAL without a launch: args, quats, image, mean_quats, status or workspace NULL, nx or ny outside [3, 2^15),
 * cos_half_tol not in (GGNN_ORIENT_H, 1] (tol outside (0, pi/2); NaN), an unknown symmetry or boundary, min_pixels < 1, max_sweeps
 * outside [0, GGNN_LABEL_MAX_SWEEPS], grain_capacity outside [1, INT32_MAX), status or workspace not 8-byte aligned, a 32-bit
 * array not 4-byte aligned, a workspace below ggnn_label_orient_workspace_bytes(nx, ny) (which is 0 for sizes the call
 * refuses).
 * A stack of maps in the same launches is ggnn_label_orientations_stack below.
 * Not covered: hexagonal and other groups, a symmetry-aware gate in ggnn_link_labels, 8-connectivity. */
#define GGNN_SYM_NONE 0
#define GGNN_SYM_CUBIC 1
#define GGNN_ORIENT_OPS 24
#define GGNN_ORIENT_H 0.70710678f
typedef struct ggnn_label_orient_args {
  const float* quats;            /* [4, ny, nx], device */
  const uint8_t* valid;          /* [ny, nx] bytes, device, or NULL: every pixel allowed */
  int32_t* image;                /* [ny, nx] out */
  float* mean_quats;             /* [4, grain_capacity] out */
  int64_t* status;               /* [GGNN_LABEL_STATUS_WORDS] out */
  void* workspace;               /* ggnn_label_orient_workspace_bytes(nx, ny) of device scratch */
  size_t workspace_bytes;
  int64_t nx, ny, grain_capacity, min_pixels;
  float cos_half_tol;            /* (float)cos((double)tol / 2) */
  int32_t symmetry;              /* GGNN_SYM_NONE / GGNN_SYM_CUBIC */
  int32_t max_sweeps;
  int32_t boundary;              /* GGNN_BC_PERIODIC / GGNN_BC_NOFLUX */
} ggnn_label_orient_args;
size_t ggnn_label_orient_workspace_bytes(int64_t nx, int64_t ny);
int ggnn_label_orientations(const ggnn_label_orient_args* args, ggnn_stream_t stream);
/* ------------------------------------------------------------------------------------
 * The two segmentations above for a STACK of T equal-shaped maps -- a recorded sequence, or an ensemble of scans that goes into
 * one union rollout -- in launches that do not grow with T.  The rule is the single call's, by reference:
 *     frame t's image, means and nine words are ggnn_label_grains' (ggnn_label_orientations') on frame t, bit for bit.
 * Frames never interact: no link, seam, vote or neighbour crosses a frame edge, and the periodic wrap of frame t goes to frame
 * t's own row 0 or column 0.  tests/labelcheck.py and tests/orientcheck.py, frame by frame, restate it.
 *   input     : T >= 1 frames of [ny, nx], N = ny nx; pixel p of frame t has index t N + p.  ids int32 [T, ny, nx] or angles
 *               float32 [T, K, ny, nx] (channel k of frame t at (t K + k) N), valid bytes [T, ny, nx] or NULL; quats float32
 *               [T, 4, ny, nx].  Every other field means what it means in the single call and holds for every frame alike
 *               (grain_capacity: rows PER FRAME).
 *   outputs   : image int32 [T, ny, nx]: ids restart in every frame (periodic from 1, no-flux from 2).  mean_angles float32
 *               [T, K, grain_capacity], row g of channel k of frame t at (t K + k) grain_capacity + g (mean_quats: K = 4);
 *               no-flux: row 0 of every frame is 0 (the identity).  Rows from a frame's n_grain on are not written.
 *               status int64 [T, GGNN_LABEL_STATUS_WORDS], zeroed by the call: row t holds frame t's nine words; n_grains,
 *               n_sweeps (the sweeps that assigned something IN FRAME t), overflow and n_bound_hits are per frame.
 *   limits    : T nx ny <= INT32_MAX (parents, roots and list entries stay int32); nx, ny in [3, 2^15).  A larger stack, or
 *               maps of different shapes, are split by the caller.  The workspace is the single call's per-frame carve times
 *               T (about 21 + 8 K bytes a pixel, 4 100 bytes of sweep words a frame), with no counter shared between
 *               workgroups; ggnn_label_stack_workspace_bytes(1, nx, ny, K) == ggnn_label_workspace_bytes(nx, ny, K).
 * ggnn_label_grains_stack = two memsets and 9 + 2 max_sweeps launches, ggnn_label_orientations_stack = two memsets and 12 + 2
 * max_sweeps launches, whatever T and whatever the maps hold: the single call's stages, each with a frame dimension (one kernel
 * body a stage; the single calls ARE the T = 1 call of the same host routine).  Tiles: T tiles workgroups.  Seams: a thread a
 * pair of every frame.  A chunk of 1 024 pixels (classify, the open lists, the sweeps, the rank) never straddles two frames:
 * ceil(N / 1 024) chunks a frame, the last one partial.  Sweeps: a word per (frame, sweep) and one per sweep summed over the
 * frames; a launch after a sweep that assigned nothing in any frame returns on the summed word without walking a list, and the
 * chunks of a frame that has gone quiet are skipped on the frame's word.  Rank: the scan of the block sums is one workgroup a
 * frame.  Counters: a wave whose lanes lie in several frames (N no multiple of 64) issues an atomic a lane into each lane's own
 * row, a wave inside one frame one atomic.  The budgets of the parent walks are those of ONE frame (4 x 1 024 hops in a tile,
 * 2 N + 64 in a seam, N + 1 in flatten).  No kernel waits on another workgroup; parent words that another workgroup may write in
 * the same launch are touched with agent-scope atomics alone; nothing outside the named arrays is addressed, whatever the inputs
 * hold; the call can be captured, and a replay gives the same bits.
 * GGNN_EINVAL without a launch: everything ggnn_label_grains (ggnn_label_orientations) refuses, T < 1, T nx ny > INT32_MAX, a
 * workspace below ggnn_label_stack_workspace_bytes(T, nx, ny, K) (ggnn_label_orient_stack_workspace_bytes(T, nx, ny)), which is
 * 0 for what the call refuses.
 * Not covered: stacks of mixed shapes, stacks beyond INT32_MAX pixels (no automatic splitter), 8-connectivity. */
typedef struct ggnn_label_stack_args {
  const int32_t* ids;            /* [T, ny, nx], device, or NULL */
  const float* angles;           /* [T, K, ny, nx], device, or NULL: exactly one of the two */
  const uint8_t* valid;          /* [T, ny, nx] bytes, device, or NULL: every pixel allowed */
  int32_t* image;                /* [T, ny, nx] out */
  float* mean_angles;            /* [T, K, grain_capacity] out (NULL with ids) */
  int64_t* status;               /* [T, GGNN_LABEL_STATUS_WORDS] out */
  void* workspace;               /* ggnn_label_stack_workspace_bytes(T, nx, ny, K) of device scratch */
  size_t workspace_bytes;
  int64_t T;
  int64_t nx, ny, grain_capacity, min_pixels;
  float tol;
  int32_t K;                     /* channels of angles; 0 with ids */
  int32_t max_sweeps;
  int32_t boundary;              /* GGNN_BC_PERIODIC / GGNN_BC_NOFLUX */
} ggnn_label_stack_args;
size_t ggnn_label_stack_workspace_bytes(int64_t T, int64_t nx, int64_t ny, int32_t K);
int ggnn_label_grains_stack(const ggnn_label_stack_args* args, ggnn_stream_t stream);
typedef struct ggnn_label_orient_stack_args {
  const float* quats;            /* [T, 4, ny, nx], device */
  const uint8_t* valid;          /* [T, ny, nx] bytes, device, or NULL: every pixel allowed */
  int32_t* image;                /* [T, ny, nx] out */
  float* mean_quats;             /* [T, 4, grain_capacity] out */
  int64_t* status;               /* [T, GGNN_LABEL_STATUS_WORDS] out */
  void* workspace;               /* ggnn_label_orient_stack_workspace_bytes(T, nx, ny) of device scratch */
  size_t workspace_bytes;
  int64_t T;
  int64_t nx, ny, grain_capacity, min_pixels;
  float cos_half_tol;            /* (float)cos((double)tol / 2) */
  int32_t symmetry;              /* GGNN_SYM_NONE / GGNN_SYM_CUBIC */
  int32_t max_sweeps;
  int32_t boundary;              /* GGNN_BC_PERIODIC / GGNN_BC_NOFLUX */
} ggnn_label_orient_stack_args;
size_t ggnn_label_orient_stack_workspace_bytes(int64_t T, int64_t nx, int64_t ny);
int ggnn_label_orientations_stack(const ggnn_label_orient_stack_args* args, ggnn_stream_t stream);
/* ------------------------------------------------------------------------------------
 * Grain ids that PERSIST across a sequence of labelled maps: ggnn_label_grains numbers every frame by the raster order of its
 * grains' first pixels, so the numbering changes as soon as a boundary moves or a grain vanishes, and ggnn_track_targets needs
 * the same grain to carry the same id in every frame.  This call links the grains of consecutive frames by their pixel
 * overlap and renumbers the whole stack, on `stream`, nothing through the host, exact in integers; tests/linkcheck.py restates
 * the rule.
 *   input     : labels int32 [T, ny, nx], T >= 1, frame t as ggnn_label_grains writes it (or any labelling with the same id
 *               ranges).  first = 1 (GGNN_BC_PERIODIC) or 2 (GGNN_BC_NOFLUX: id 1 is the boundary grain and maps to itself).
 *               n_local int64 [T] ON THE DEVICE (word 4 of a labelling's status: no read-back between the two calls); L_t =
 *               n_local[t] clamped to [0, local_capacity].  The local grains of frame t are the ids first .. first + L_t - 1.
 *               Pixel 0 is unfilled: it never votes and stays 0.  Every other id outside these (negative, or at or beyond
 *               first + L_t, so anything at or beyond first + local_capacity) is treated as 0 and counted in `overflow`, a
 *               pixel each; a frame with n_local[t] outside [0, local_capacity] counts once more.
 *               means (optional, K > 0) float32 [T, K, local_capacity]: row b - first of frame t and channel k, at
 *               (t K + k) local_capacity + b - first, is the mean of local grain b.
 *   votes     : for t >= 1 and every pixel p, a = labels[t-1][p], b = labels[t][p]; when both are local grains of their
 *               frames, vote(t, b, a) += 1.  Integers: exact whatever the order.
 *   candidates: grain a of frame t - 1 is ELIGIBLE for grain b of frame t when vote(t, b, a) >= min_overlap (>= 1) and, when
 *               the gate is on (use_match_tol, K > 0), fabsf(mean[t][k][b] - mean[t-1][k][a]) <= match_tol in every channel --
 *               one fp32 subtraction each, the form of ggnn_label_grains' tol (a NaN fails it).
 *   pred      : pred(t, b) = the eligible a with the most votes, a tie going to the smaller a; -1 when there is none, and in
 *               frame 0.
 *   claims    : among the b of frame t with pred(t, b) = a, the one with the largest vote(t, b, a) keeps it, a tie going to the
 *               smaller b; every other claimant gets pred = -1 and counts in n_split.  A grain of frame t - 1 that nobody keeps
 *               counts in n_gone of frame t.
 *   global ids: gid(0, b) = b; gid(t, b) = gid(t-1, pred(t, b)) when pred >= 0; otherwise the grain is FRESH: fresh grains are
 *               numbered from first + L_0 on, by ascending frame and then ascending local id.  n_global = L_0 + the number of
 *               fresh grains (no-flux: the sequence has n_global + 1 grains, as ggnn_label_grains counts).  A grain pinched in
 *               two keeps its id on the larger part; nothing merges ids; a grain that is absent from one frame and present in
 *               the next comes back FRESH, under a new id; only frame t - 1 is looked at.
 *   outputs   : frames_out int32 [T, ny, nx]: gid(t, labels[t][p]), 0 -> 0, no-flux 1 -> 1 (must not alias labels).
 *               gid, pred int32 [T, local_capacity], row b - first; rows from L_t on: 0 and -1.
 *               first_frame, last_frame int32 [global_capacity], row g - first of global grain g: the first frame that holds
 *               it and the last of the unbroken run that does; theta (K > 0) float32 [K, global_capacity]: the grain's mean
 *               in its first frame, copied, not recomputed.  Rows from n_global on: -1, -1 and 0.
 *               n_global > global_capacity adds 1 to `overflow`: the images are still complete, the per-grain rows hold the
 *               first global_capacity grains.
 *   status    : int64 [GGNN_LINK_FRAME_WORDS T + GGNN_LINK_GLOBAL_WORDS], zeroed by the call.  Per frame t, at
 *               GGNN_LINK_FRAME_WORDS t: n_local (L_t), n_matched, n_fresh (the split ones included; 0 in frame 0), n_split,
 *               n_gone, n_vote_overflow; then n_global and overflow.
 * ggnn_link_labels = at most six memsets and five launches (three with T = 1: there is no pair to vote on), whatever T > 1
 * and whatever the images hold:
 *   votes     every (frame t >= 1, local grain) owns GGNN_LINK_SLOTS slots of (key a, count) in the workspace.  A thread takes
 *             GGNN_LINK_RUN consecutive pixels of a row, merges equal consecutive (b, a) pairs and spends one probe of at most
 *             GGNN_LINK_SLOTS slots a distinct pair: atomicCAS on the key, atomicAdd on the count.  A vote that finds
 *             GGNN_LINK_SLOTS other keys is dropped and its pixels are counted in n_vote_overflow of its frame: the results are
 *             defined only when that word is 0 in every frame (a grain that overlaps more than GGNN_LINK_SLOTS grains of the
 *             frame before: the frames are too far apart).
 *   match     a thread per (t, b): the slots, the gates, the argmax; a 64-bit atomicMax of (vote << 32) | (0xFFFFFFFF - b) on
 *             the claim word of (t - 1, a): the winner does not depend on the order.
 *   resolve   a thread per (t, b) keeps pred only if the claim word names it; n_split, n_gone; the unused rows.
 *   compose   one workgroup walks t = 0 .. T - 1 over grain rows, a block scan over the fresh flags in chunks; n_global.
 *   relabel   a thread per pixel.
 * No kernel waits on another workgroup; every loop is bounded by T, local_capacity and the pixels; nothing outside the named
 * arrays is addressed, whatever the inputs hold; counters are integer atomics and no result is ordered by one; the call can
 * be captured, and a replay gives the same bits.
 * GGNN_EINVAL without a launch: args, labels, n_local, frames_out, gid, pred, first_frame, last_frame, status or workspace
 * NULL, T < 1, nx or ny outside [3, 2^15), local_capacity or global_capacity outside [1, INT32_MAX), T local_capacity beyond
 * 2^36, K outside [0, 4], with K > 0 means or theta NULL, min_overlap < 1, use_match_tol with K = 0 or with match_tol not
 * >= 0, an unknown boundary, n_local, status or workspace not 8-byte aligned, a 32-bit array not 4-byte aligned, a workspace
 * below ggnn_link_workspace_bytes(T, local_capacity, K) (which is 0 for sizes the call refuses).
 * Not covered: merging grains (two grains that become one: the smaller one is gone), a grain that reappears keeping its id,
 * matching across more than one frame back, crystal symmetry in the gate.  (The stack itself is labelled in launches that do
 * not grow with T by ggnn_label_grains_stack / ggnn_label_orientations_stack above.) */
#define GGNN_LINK_SLOTS 16
#define GGNN_LINK_RUN 4
#define GGNN_LINK_FRAME_WORDS 6
#define GGNN_LINK_GLOBAL_WORDS 2
typedef struct ggnn_link_labels_args {
  const int32_t* labels;         /* [T, ny, nx], device */
  const int64_t* n_local;        /* [T], device */
  const float* means;            /* [T, K, local_capacity], device, or NULL with K = 0 */
  int32_t* frames_out;           /* [T, ny, nx] out */
  int32_t* gid;                  /* [T, local_capacity] out */
  int32_t* pred;                 /* [T, local_capacity] out */
  int32_t* first_frame;          /* [global_capacity] out */
  int32_t* last_frame;           /* [global_capacity] out */
  float* theta;                  /* [K, global_capacity] out (NULL with K = 0) */
  int64_t* status;               /* [GGNN_LINK_FRAME_WORDS T + GGNN_LINK_GLOBAL_WORDS] out */
  void* workspace;               /* ggnn_link_workspace_bytes(T, local_capacity, K) of device scratch */
  size_t workspace_bytes;
  int64_t T, nx, ny, local_capacity, global_capacity, min_overlap;
  float match_tol;
  int32_t use_match_tol;         /* 0: overlap alone */
  int32_t K;                     /* channels of means */
  int32_t boundary;              /* GGNN_BC_PERIODIC / GGNN_BC_NOFLUX */
} ggnn_link_labels_args;
size_t ggnn_link_workspace_bytes(int64_t T, int64_t local_capacity, int32_t K);
int ggnn_link_labels(const ggnn_link_labels_args* args, ggnn_stream_t stream);
/* The host-side topology update those counts trigger: one call of the reference's `Cmodel.update`
 * (models.py:612-842 with delete_grain_index :861-893, switching_edge_index :896-1051, point_in_triangle :1055-1070,
 * periodic_move :1103-1106), nucleation off.  HOST memory throughout, no stream: grains of `grain_event` (those below the
 * area threshold, smallest first, test.py:418-420) are eliminated, junction edges with edge_prob > threshold are switched
 * (most probable first), grains left with two junctions are removed.  Bit-exact contract: the edge lists keep the
 * reference's COLUMN ORDER (columns rewritten in place, new columns appended, dead columns dropped at the end), masks and
 * fp32 junction coordinates are the reference's.
 *   pp, pq      : [2][cap] int64 junction->junction / junction->grain lists (row r at pp + r * pp_cap), n_pp / n_pq columns in
 *                 use; updated IN PLACE, n_pp / n_pq = the new column counts.  pp_cap >= n_pp + 2 (removed grains): every
 *                 removed grain appends two columns before the dead ones are dropped.
 *   x_joint     : [n_joint, ldx >= 8] fp32, columns 0, 1 (position) and 6, 7 (displacement feature) are rewritten for the
 *                 junctions an event moves; y_joint [n_joint, 2] likewise
 *   y_grain_area: element g at y_grain_area[g * ldyg] (the regressor's y_grain[:, 0]);  edge_prob [n_pp] = sigmoid(edge_event)
 *   mask_grain / mask_joint : [n] int64, 1 = live; eliminated grains and their junctions are cleared
 *   active_grain / active_joint : optional [n] bytes, 0 = outside the active window (models.py:640-645, 911): frozen
 *   switching   : out [switching_cap][2] the switched junction pairs, n_switching of them
 *   events_extra: out [extra_cap] grains eliminated beyond `grain_event` (forced / two-sided), n_extra of them
 * Returns GGNN_OK, GGNN_EINVAL, or GGNN_ETOPOLOGY with a message in `error` (the reference asserts / raises there); on an error
 * the in/out arrays are in an undefined state: pass copies (graingraphnn_amd/topology.py does).  The room of the output lists
 * (switching_cap >= the edges above the threshold, extra_cap >= n_grain + 1) is checked before anything is rewritten.
 * Refusals where the reference would raise an IndexError of its own (reachable on degenerate lists only): a junction with
 * fewer than three grain columns or fewer than two other neighbours in a switch.  (A junction pair of an eliminated grain
 * joined by MORE than one column is not refused: the reference indexes the concatenated hits with the order of the edges all
 * the same, and so does this -- rounds 5-6 refused there, one step before the reference's formulation failed by itself.) */
typedef struct ggnn_topology_args {
  int64_t* pp;
  int64_t* pq;
  int64_t n_pp, n_pq, pp_cap, pq_cap;
  float* x_joint;
  float* y_joint;
  const float* y_grain_area;
  const float* edge_prob;
  const int64_t* grain_event;
  int64_t* mask_grain;
  int64_t* mask_joint;
  const uint8_t* active_grain;
  const uint8_t* active_joint;
  int64_t* switching;
  int64_t* events_extra;
  int64_t n_joint, n_grain, ldx, ldyg, n_grain_event, switching_cap, extra_cap, n_switching, n_extra;
  double threshold;
  char error[192];
} ggnn_topology_args;
int ggnn_topology_update(ggnn_topology_args* args);
/* The same update on lists that live in the library between calls (graingraphnn_amd/rollout.py keeps one session per
 * trajectory): the reference's loop calls Cmodel.update at EVERY step (test.py:418-426), and a stateless call rebuilds its
 * lookup tables from the whole lists each time (four O(E) sorts for a handful of events).  A session keeps the lists, the
 * tables and the per-grain counts and patches them as the events rewrite columns; a call costs what its events touch plus
 * one pass that renumbers the live columns.  HOST memory, no stream, one thread per session at a time.
 *   ggnn_topology_open   : pp [2][n_pp] (row r at pp + r * pp_ld), pq likewise -> *session.  GGNN_ETOPOLOGY (message in
 *                          `error`, 192 bytes, may be NULL) for an index outside [0, n_joint) / [0, n_grain).
 *   ggnn_topology_apply  : one update; of `args` pp / pq / *_cap are ignored (the session holds the lists), everything else
 *                          as for ggnn_topology_update; n_pp / n_pq = the new column counts.  A refused call
 *                          (GGNN_ETOPOLOGY) leaves the session AND x_joint / y_joint / the masks exactly as they were.
 *   ggnn_topology_export : the current lists in the reference's column order into the caller's arrays (any may be NULL):
 *                          pp [2][>= n_pp], pq [2][>= n_pq], qp = pq with its rows exchanged (the grain -> junction list,
 *                          models.py:841).
 *   ggnn_topology_counts, ggnn_topology_close. */
typedef struct ggnn_topology_session ggnn_topology_session;
int ggnn_topology_open(const int64_t* pp, int64_t n_pp, int64_t pp_ld, const int64_t* pq, int64_t n_pq, int64_t pq_ld,
                       int64_t n_joint, int64_t n_grain, ggnn_topology_session** session, char* error);
int ggnn_topology_apply(ggnn_topology_session* session, ggnn_topology_args* args);
int ggnn_topology_counts(const ggnn_topology_session* session, int64_t* n_pp, int64_t* n_pq);
int ggnn_topology_export(const ggnn_topology_session* session, int64_t* pp, int64_t pp_ld, int64_t* pq, int64_t pq_ld,
                         int64_t* qp, int64_t qp_ld);
void ggnn_topology_close(ggnn_topology_session* session);
typedef struct ggnn_refresh_edge {
  const int64_t* edge_index; /* [2, E] */
  const float* x_src;
  const float* x_dst;
  float* edge_attr; /* [E] out */
  int64_t ldx_src, ldx_dst, n_src, n_dst, E;
  const int64_t* E_dev;      /* NULL, or as in ggnn_prepare_edge (edge_index is [2, *E_dev] then) */
} ggnn_refresh_edge;
int ggnn_step_refresh(float* x_joint, int64_t n_joint, int64_t ldx_joint, float* x_grain,
                      int64_t n_grain, int64_t ldx_grain, float zmax, const int32_t* flags,
                      const ggnn_refresh_edge* edges, int n_edge_types, ggnn_stream_t stream);

/* ggnn_step_refresh + ggnn_edge_prepare of the NEXT forward in ONE launch: z clamp of every node when
 * flags[1] is set, then per CSR slot the edge length from the min-image xy offsets (written to
 * edge_attr[perm[p]], the COO order: edges[k].edge_attr is an OUTPUT here) and the einfo record with that
 * length.  Same values as the two calls in sequence (the length is the same expression on the same operands).
 * x_joint_mirror / x_grain_mirror (both or neither, NULL = none; same shape and leading dimension as x_joint /
 * x_grain, not x itself): every row of x as it stands behind this call (the clamped z included) is also written there --
 * the copy of the node features that the classifier's forward of the NEXT step reads (test.py:382-383 hands both models
 * the same x_dict) while Rmodel.update of that step already rewrites x in place (graingraphnn_amd/rollout.py). */
int ggnn_step_refresh_prepare(float* x_joint, int64_t n_joint, int64_t ldx_joint, float* x_grain,
                              int64_t n_grain, int64_t ldx_grain, float zmax, const int32_t* flags,
                              const ggnn_prepare_edge* edges, int n_edge_types, float* x_joint_mirror,
                              float* x_grain_mirror, ggnn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Training path: the LSTM update of HeteroPGCLSTM.forward (heteropgclstm.py:140-183) with the
 * state its backward needs, and that backward.  Replaces what autograd records for the sigmoid / tanh /
 * multiply / add chain of `i, f, c, o` (one launch each way instead of ~40).  n_gates = 4: (i, f, c, o) with
 * c_in; n_gates = 3: (i, c, o), zero state (encoder), c_in = NULL.
 *   forward : z [n_gates, N, 96] holds the gate GEMM's output (lin_l2 part) on entry; on exit the
 *             pre-activations z_g = gemm_g + p_dst[n, s_off + g*96 ..] (skip rows of ggnn_project_batch); writes
 *             h_out, c_out [N, 96].
 *   backward: g_h / g_c (gradients of h_out / c_out; NULL = zero) -> g_z [n_gates, N, 96], the same values
 *             into g_p_dst[n, s_off + g*96 ..] (gradient of the skip rows; NULL = skip), g_c_in (NULL = skip).
 * ldp % 4 == 0, s_off % 4 == 0, every pointer 16-byte aligned.
 * The node types of a cell (1..GGNN_LSTM_TRAIN_MAX problems of one gate count) in ONE launch each way.  The forward reads
 * (z, p_dst, ldp, s_off, c_in) and writes (z, h_out, c_out); the backward reads (z, c_in, c_out, g_h, g_c) and writes
 * (g_z, g_p_dst, g_c_in).  Backward only: it also writes zeros into g_p_dst[n, pad_off .. pad_off + pad_n) (the
 * projection gradient's padding columns, which no kernel of the cell's backward writes and the weight gradient reads:
 * pad_off % 4 == 0, pad_n % 4 == 0, pad_n <= 96; 0 = nothing). */
#define GGNN_LSTM_TRAIN_MAX 4
typedef struct ggnn_lstm_train_problem {
  float* z;
  const float* p_dst;
  const float* c_in;
  float* h_out;
  float* c_out;
  const float* g_h;
  const float* g_c;
  float* g_z;
  float* g_p_dst;
  float* g_c_in;
  int64_t ldp, N;
  int32_t s_off, pad_off, pad_n, reserved;
} ggnn_lstm_train_problem;
int ggnn_lstm_train_forward_batch(const ggnn_lstm_train_problem* problems, int n_problems, int n_gates, ggnn_stream_t stream);
int ggnn_lstm_train_backward_batch(const ggnn_lstm_train_problem* problems, int n_problems, int n_gates, ggnn_stream_t stream);

/* Training path: backward of ggnn_heads_regressor.  From the gradients of (y_joint [n_joint, 2], y_grain [n_grain, 2],
 * grain_area [n_grain]; any may be NULL = zero) and the forward's saved y_joint / y_grain: g_pre_* [n, 4] = gradient of
 * the heads' pre-activations (columns 2-3 zero: the operand of ggnn_wgrad for the head weights and biases) and
 * g_h_* [n, 96] = g_pre W.  w as in the forward. */
int ggnn_heads_regressor_backward(int64_t n_joint, int64_t n_grain, const float* w, const float* y_joint,
                                  const float* y_grain, const float* g_y_joint, const float* g_y_grain,
                                  const float* g_grain_area, float* g_pre_joint, float* g_pre_grain,
                                  float* g_h_joint, float* g_h_grain, ggnn_stream_t stream);

/* Weight-gradient GEMM of the training path: C[b] = A[b]^T B[b] with a long reduction (K = nodes) and a small
 * M x Nc result -- the gradient of a packed projection ([ncols, F + 97]) or gate ([96, Kg] per gate) weight
 * matrix, replacing the BLAS call autograd would make for x.t() @ g (which does not split K).  The reduction is
 * split over the chip in a fixed way; the call writes partial[s][b][M][Nc], s < ggnn_wgrad_splits(K, M, Nc, batch),
 * and sums over s into `out` (in index order; out == NULL: left to the caller).  Arithmetic: fp32-equivalent over fp32's
 * whole range either way -- exact fp32 products (v_mfma_f32_16x16x4_f32) for the short results, and for the TALL ones
 * (M >= 512: the packed projection's gradient) under the default GEMM mode both operands as three exact bf16 pieces with
 * six products per k-step (2e-8 of sum |a||b| against an fp64 product; gradients of 1e-10 keep their 24 bits, which a
 * two-piece fp16 split would not give them).  M, Nc, lda, ldb, a_bstride, b_bstride multiples of 4 (pad B with zero columns
 * otherwise); a, b 16-byte aligned.
 * b_ins != NULL: B is `b` with the ins_w columns of `b_ins` [K, ld_ins] INSERTED at column ins_off -- column c of B is
 * b[c] for c < ins_off, b_ins[c - ins_off] for the next ins_w columns, b[c - ins_w] behind them (Nc counts all of them; b holds
 * Nc - ins_w columns) -- so that the weight gradient of a projection reads [x | 0 | h | 1 0 0 0] from the data skeleton
 * [x | 0 | 1 0 0 0] (ggnn_train_input_rows, once per step) and the hidden state where it lies, without a concatenated copy.
 * ins_off, ins_w, ld_ins multiples of 4, b_ins 16-byte aligned, batch == 1. */
typedef struct ggnn_wgrad_args {
  const float* a;  /* [batch] x [K, lda] row-major, first M columns used; batch b starts at a + b * a_bstride */
  const float* b;  /* [batch] x [K, ldb], first Nc columns used; batch b starts at b + b * b_bstride */
  float* partial;  /* [n_split, batch, M, Nc] out */
  float* out;      /* [batch, M, Nc] out: the sum over the splits, or NULL (16-byte aligned) */
  int64_t lda, ldb, a_bstride, b_bstride, K;
  int32_t M, Nc, batch, n_split;
  const float* b_ins;  /* or NULL */
  int64_t ld_ins;
  int32_t ins_off, ins_w;
} ggnn_wgrad_args;
int ggnn_wgrad_splits(int64_t K, int M, int Nc, int batch);
int ggnn_wgrad(const ggnn_wgrad_args* args, ggnn_stream_t stream);

/* Training path: the data part of the weight gradients' B operands, for the node types of a step in one launch:
 * out[n, 0 .. Fp + 4) = [x[n, 0 .. F) | 0 .. (Fp - F zeros) | 1 0 0 0], Fp = F rounded up to 4 -- what the encoder's projection
 * gradient multiplies with as it is, and the decoder's with the hidden state inserted at column Fp (ggnn_wgrad, b_ins).
 * out 16-byte aligned, ldo >= Fp + 4, ldo % 4 == 0; 3 <= F <= 12. */
#define GGNN_TRAIN_ROWS_MAX 4
typedef struct ggnn_train_rows_problem {
  const float* x;
  float* out;
  int64_t ldx, ldo, N;
  int32_t F, reserved;
} ggnn_train_rows_problem;
int ggnn_train_input_rows(const ggnn_train_rows_problem* problems, int n_problems, ggnn_stream_t stream);

/* Training path: out[b][j] = sum_r in[b][r][j], b < batch -- the caller's reduction over the partial sums of
 * ggnn_period_gat_aggregate_backward (ep_partial: n_rows = ggnn_aggregate_bwd_partials rows of n_cols = n_gates * 288 floats
 * per edge type), in a fixed order.  in: [batch, n_rows, n_cols] contiguous, n_cols % 4 == 0, 16-byte aligned. */
int ggnn_sum_rows(const float* in, float* out, int64_t n_rows, int64_t n_cols, int32_t batch, ggnn_stream_t stream);
/* 1..GGNN_SUM_ROWS_MAX such sums in one launch, each with its own shape -- the reductions a cell's backward pass can
 * postpone to its end: the split-K partials of its weight gradients (ggnn_wgrad with out == NULL: in = partial, n_rows =
 * n_split, n_cols = batch M Nc, batch = 1) and the edge-parameter partials of its sweeps.  Same fixed summation tree as
 * ggnn_sum_rows (32 interleaved row groups, combined in index order). */
#define GGNN_SUM_ROWS_MAX 8
typedef struct ggnn_sum_rows_problem {
  const float* in;   /* [batch, n_rows, n_cols] contiguous, 16-byte aligned */
  float* out;        /* [batch, n_cols] */
  int64_t n_rows, n_cols;
  int32_t batch, reserved;
} ggnn_sum_rows_problem;
int ggnn_sum_rows_batch(const ggnn_sum_rows_problem* problems, int n_problems, ggnn_stream_t stream);

/* Training path: the nine packed weight matrices of a cell (projection weights and biases of both node types, relocation
 * columns per edge type, gate weights: graingraphnn_amd/packing.py) from its parameters, differentiable -- the device side of
 * train_pack._PackWeights.  The packing is described by index tables (train_pack.PackPlan): with
 *   flat2 = [ the cell's parameters, concatenated (n_flat) | nb products [r, c] | one zero slot ],  zero = n_flat + nb r c,
 * every packed entry is the sum of L elements of flat2 (idx3 [n_packed, L]; the index `zero` reads 0), and product b is
 * (coef K_b) Q_b with K_b [r, 96], Q_b [96, c] themselves gathered from flat2: kq_idx = [K entries (nb r 96) | Q entries
 * (nb 96 c)].  ggnn_pack_weights_batch: the caller has written the parameters to flat2[0 .. n_flat); the call fills the products
 * and `packed`.  ggnn_pack_weights_backward_batch: g_out[s] = gradient of output s (NULL: zero), output s being
 * packed[g_off[s] .. g_off[s + 1]); inv [n_flat2, inv_m] = the packed entries that read each element of flat2 (padding:
 * n_packed), inv_kq [n_flat, inv_kq_m] = the operand entries that read each parameter (padding: n_kq = nb 96 (r + c));
 * g_flat2 [n_flat2] and g_kq [n_kq] are workspaces, g_flat [n_flat] receives the parameters' gradient.  Plain fp32 fmas. */
#define GGNN_PACK_OUTPUTS 9
typedef struct ggnn_pack_args {
  float* flat2;
  float* kq;                /* [nb 96 (r + c)] the products' operands gathered from flat2 (K side x coef): written by the forward, read by the backward */
  const int64_t* kq_idx;
  const int64_t* idx3;
  float* packed;
  int64_t n_flat, zero, n_packed;
  int32_t nb, r, c, L;
  float coef;
  int32_t reserved;
  const float* const* params;   /* NULL, or the DEVICE array of the parameter tensors' addresses.  With it the entries of kq_idx
                                   and idx3 that address a parameter are ENCODED as ((t + 1) << GGNN_PACK_TENSOR_SHIFT) | (offset
                                   inside tensor t) and read from params[t] where the tensor lies (flat2[0 .. n_flat) is then not
                                   read: no concatenated copy of the parameters); entries >= n_flat (products, zero slot) stay
                                   plain flat2 indices.  NULL: every entry is a plain flat2 index. */
} ggnn_pack_args;
#define GGNN_PACK_TENSOR_SHIFT 40
typedef struct ggnn_pack_bwd_args {
  ggnn_pack_args fwd;                       /* as in the forward call (packed is not used) */
  const float* g_out[GGNN_PACK_OUTPUTS];
  int64_t g_off[GGNN_PACK_OUTPUTS + 1];
  int64_t g_w[GGNN_PACK_OUTPUTS], g_rs[GGNN_PACK_OUTPUTS], g_cs[GGNN_PACK_OUTPUTS];   /* element e of output s = g_out[s][(e / w) rs + (e % w) cs]: a
                                                                                         contiguous gradient is (w = its size, rs = 0, cs = 1), a column
                                                                                         block of a wider matrix (w = its width, rs = the row stride) */
  const int64_t* inv;
  const int64_t* inv_kq;
  float* g_flat2;
  float* g_kq;
  float* g_flat;
  int64_t n_flat2, n_kq;
  int32_t inv_m, inv_kq_m;
  int64_t n_tail;   /* g_flat has n_flat + n_tail elements; the tail is written with zeros (the gradient of the parameters
                       the reference's forward reads without effect: the encoder's forget gate) */
} ggnn_pack_bwd_args;
/* 1..GGNN_PACK_MAX cells per call (the encoder's and the decoder's of a training step) with every launch shared: three
 * launches forward and four backward whatever the number of cells (each of these kernels is a few microseconds of latency
 * on ~1 MB of data). */
#define GGNN_PACK_MAX 2
int ggnn_pack_weights_batch(const ggnn_pack_args* args, int n_cells, ggnn_stream_t stream);
int ggnn_pack_weights_backward_batch(const ggnn_pack_bwd_args* args, int n_cells, ggnn_stream_t stream);

/* Training path: torch.optim.Adam's update (train.py:82-91; amsgrad / maximize off) for up to GGNN_ADAM_MAX_TENSORS parameter
 * tensors in one launch.  `table` (DEVICE memory, n_tensors entries, built once) holds what is fixed: the addresses of a
 * parameter and its two moment buffers, its size, its parameter group.  Workgroup c of the launch updates elements
 * [chunk_index[c] * GGNN_ADAM_CHUNK, +GGNN_ADAM_CHUNK) of tensor chunk_tensor[c] (DEVICE arrays of n_chunks entries, built once
 * from the sizes).  What changes per step comes by value: grad[t] (NULL: tensor t is skipped), lr / weight_decay per group --
 * or, with `hyper` set, lr and weight_decay are read from DEVICE memory (hyper[g] = lr of group g, hyper[GGNN_ADAM_MAX_GROUPS + g]
 * = its weight_decay): a call captured in a hipGraph then follows a learning-rate schedule (train.py:91, StepLR) through
 * an uncaptured copy into that array between replays, where by-value arguments would replay the captured rates for ever.
 * step (DEVICE, n_tensors floats, 0 before the first call): step[t] = updates tensor t has had so far -- read for the bias
 * corrections and incremented by the call itself (a second small launch) where grad[t] != NULL (torch keeps a count per
 * parameter: one without a gradient does not advance), so a captured call replays correctly.  A model with more tensors
 * takes several calls per update, each on its own slice of the table and of step.  Per element:
 *   g += weight_decay p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
 *   p -= lr / (1 - b1^s) * m / (sqrt(v) / sqrt(1 - b2^s) + eps),   s = step[t] + 1. */
#define GGNN_ADAM_CHUNK 4096
#define GGNN_ADAM_MAX_TENSORS 384
#define GGNN_ADAM_MAX_GROUPS 8
typedef struct ggnn_adam_tensor {
  float* param;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t n;
  int32_t group, reserved;
} ggnn_adam_tensor;
typedef struct ggnn_adam_args {
  const ggnn_adam_tensor* table;
  const int32_t* chunk_tensor;
  const int32_t* chunk_index;
  float* step;
  const float* grad[GGNN_ADAM_MAX_TENSORS];
  float lr[GGNN_ADAM_MAX_GROUPS], weight_decay[GGNN_ADAM_MAX_GROUPS];
  float beta1, beta2, eps;
  int32_t n_chunks, n_tensors;
  const float* hyper;   /* optional, DEVICE: [2][GGNN_ADAM_MAX_GROUPS] lr | weight_decay per group, read instead of the by-value ones */
} ggnn_adam_args;
int ggnn_adam_step(const ggnn_adam_args* args, ggnn_stream_t stream);

/* Training path: the regressor's loss (train.py:31-37, edge_len off) with its gradient in one launch:
 *   loss = scale * sum_k mean_i(mask_k[i / mask_div_k] (pred_k[i] - target_k[i])^2),   g_pred_k[i] = d loss / d pred_k[i]
 * over n_terms <= GGNN_MSE_MAX_TERMS terms of n[k] elements (mask NULL = ones; mask_div = elements of pred per mask entry;
 * g_pred NULL = not wanted).  workspace: GGNN_MSE_BLOCKS + 1 doubles of DEVICE memory, zero before the first call (the call
 * leaves its last entry zero again).  The sum is taken in a fixed order. */
#define GGNN_MSE_MAX_TERMS 4
#define GGNN_MSE_BLOCKS 64
typedef struct ggnn_mse_args {
  const float* pred[GGNN_MSE_MAX_TERMS];
  const float* target[GGNN_MSE_MAX_TERMS];
  const float* mask[GGNN_MSE_MAX_TERMS];
  float* g_pred[GGNN_MSE_MAX_TERMS];
  int64_t n[GGNN_MSE_MAX_TERMS];
  int64_t mask_div[GGNN_MSE_MAX_TERMS];
  double* workspace;
  float* loss; /* [1] out */
  float scale;
  int32_t n_terms;
} ggnn_mse_args;
int ggnn_masked_mse(const ggnn_mse_args* args, ggnn_stream_t stream);
/* The same launch for terms whose tensors carry pad rows behind the real ones (a batch buffer of capacity shape,
 * ggnn_collate_batch): the mean of term k is taken over *rows[k] * row_elems[k] elements, read at RUN time, where rows[k] is
 * not NULL -- the sum still walks all n[k] elements, so the pad rows must add exact zeros (mask 0, finite operands).
 * rows[k] NULL (or counts NULL) = n[k]: ggnn_masked_mse.  A count <= 0 makes the term and its gradient zero. */
typedef struct ggnn_mse_counts {
  const int64_t* rows[GGNN_MSE_MAX_TERMS]; /* DEVICE [1] each, or NULL */
  int64_t row_elems[GGNN_MSE_MAX_TERMS];
} ggnn_mse_counts;
int ggnn_masked_mse_rows(const ggnn_mse_args* args, const ggnn_mse_counts* counts, ggnn_stream_t stream);

/* Training on device-resident mini-batches.  The dataset lives in ARENAS: per array kind the rows of all samples
 * one after another, per-sample offsets sample_off[kind][n_samples + 1]; a sample's edge indices are local to it.
 * ggnn_collate_batch = the collation of train.py:365-366 (PyG DataLoader: node rows concatenated, edge indices offset by the
 * node counts of the samples in front) in ONE launch: with b = *cursor_in modulo n_batches and the sample ids
 * order[b * batch_size .. + batch_size) (-1 = an empty slot)
 *   rows[j]   a row array of `words` 4-byte words per row (features, targets, masks, edge attributes, labels: any dtype of
 *             4 or 8 bytes): dst holds the batch's rows from row 0, every word of the rows behind them is pad_word;
 *   lists[j]  an edge list: dst [2][cap] = the samples' lists, sources shifted by the slot's first row of kind_src,
 *             destinations by that of kind_dst; the edges behind them are (pad_src, pad_dst) -- two rows the caller keeps
 *             free of real nodes and masks out of the tables (ggnn_csr_mask); dst_flipped (optional) the same list with the
 *             two rows swapped (the list of the reverse table);
 *   count[kind] = the batch's real rows / edges, batch_off[kind][batch_size + 1] = the first row / edge of every slot
 *             (written by the array with meta = 1 of a node kind, by the list of an edge kind).
 * The pad is rewritten by every call.  The grid depends on the capacities only; nothing is allocated, no floating-point or
 * data atomics: an integer ticket (sync_word, zero before the first call and left zero) lets the last workgroup store
 * *cursor_out = *cursor_in + 1, which may be the same word -- a replayed hipGraph moves on to the next batch by itself.
 * The caller guarantees that every batch fits (capacities from the batch_size largest samples) and that the arenas hold
 * what sample_off says; ids outside [0, n_samples) are empty slots.  GGNN_EINVAL without a launch: NULL operands, sizes
 * outside their ranges, kinds outside [0, n_kinds). */
#define GGNN_COLLATE_MAX_BATCH 64
#define GGNN_COLLATE_MAX_ROWS 12
#define GGNN_COLLATE_MAX_LISTS 3
#define GGNN_COLLATE_MAX_KINDS 5
typedef struct ggnn_collate_rows {
  const uint32_t* src;
  uint32_t* dst;
  int64_t cap;       /* rows of dst */
  int32_t words;     /* 1 .. 64 */
  int32_t kind;
  uint32_t pad_word;
  int32_t meta;      /* 1: this array's launch share also writes count[kind] and batch_off[kind] */
} ggnn_collate_rows;
typedef struct ggnn_collate_list {
  const int64_t* src;   /* [2][ld_src] */
  int64_t* dst;         /* [2][cap] */
  int64_t* dst_flipped; /* [2][cap] or NULL */
  int64_t ld_src, cap;
  int64_t pad_src, pad_dst;
  int32_t kind, kind_src, kind_dst, reserved;
} ggnn_collate_list;
typedef struct ggnn_collate_args {
  const int64_t* sample_off[GGNN_COLLATE_MAX_KINDS];
  int64_t* batch_off[GGNN_COLLATE_MAX_KINDS];
  int64_t* count[GGNN_COLLATE_MAX_KINDS];
  const int32_t* order; /* [n_batches][batch_size] */
  const int32_t* cursor_in;
  int32_t* cursor_out;
  int32_t* sync_word;
  ggnn_collate_rows rows[GGNN_COLLATE_MAX_ROWS];
  ggnn_collate_list lists[GGNN_COLLATE_MAX_LISTS];
  int64_t n_samples;
  int32_t n_batches, batch_size, n_kinds, n_rows, n_lists, reserved;
} ggnn_collate_args;
int ggnn_collate_batch(const ggnn_collate_args* args, ggnn_stream_t stream);

/* r_slot[q] = the forward CSR slot of the edge in reverse (source-grouped) CSR slot q, for tables of which only the first
 * *E_kept slots are filled (masked builds; E_kept NULL = E): perm / r_perm = the two tables' slot -> original edge maps
 * ([E] int32, ggnn_csr_args.perm), scratch [E] int32; r_slot[q >= *E_kept] = 0.  Up to GGNN_COLLATE_MAX_LISTS lists per call,
 * two launches, no read-back. */
typedef struct ggnn_reverse_slots_args {
  const int32_t* perm;
  const int32_t* r_perm;
  int32_t* r_slot;
  int32_t* scratch;
  const int64_t* E_kept; /* DEVICE [1] or NULL */
  int64_t E;
} ggnn_reverse_slots_args;
int ggnn_reverse_slots(const ggnn_reverse_slots_args* lists, int n_lists, ggnn_stream_t stream);

/* Validation metrics (metrics.py:23-72 feature_metric.record, :124-217 grain_class_acc / class_acc): ONE launch adds one
 * validation batch to a device-resident accumulator; nothing is read back before the epoch's summary.
 *   squared-error terms k < n_terms <= GGNN_METRIC_MAX_TERMS over n_rows[k] rows, m = mask[k][r ld_mask[k]]:
 *       acc.f64[k]     += sum_r m (target[k][r ld[k] + col[k]] - pred[k][r ld[k] + col[k]])^2
 *       acc.f64[4 + k] += sum_r m  target[k][r ld[k] + col[k]]^2                          (only with with_norm != 0)
 *     fp32 inputs; the difference, the squares and the sums are fp64.  A row with m == 0 contributes EXACTLY 0 to both,
 *     even where pred or target is not finite (the reference's 0 * inf is NaN there; classifier_loss makes the same choice).
 *   one threshold term of n elements (score fp32, label int64 read as stored, optional row mask label_mask[i ld_label_mask]),
 *     n_thr <= GGNN_METRIC_MAX_THR thresholds thr[] compared in fp32:
 *       GGNN_METRIC_CLASSIFIER  counted: label > -1;     s = 1 / (1 + exp(-score)) in fp32;  positive: s > t;  negative: s <= t
 *       GGNN_METRIC_REGRESSOR   counted: label_mask > 0; s = score;                          positive: s < t;  negative: s >= t
 *       acc.i64[j] += #(label == 1, positive)   acc.i64[16 + j] += #(label == 0, positive)   acc.i64[32 + j] += #(label == 1, negative)
 *     (a label that is neither 0 nor 1 counts nowhere)
 *   loss != NULL: acc.f64[8] += (double)*loss (a DEVICE float) and acc.i64[48] += 1.
 * acc: GGNN_METRIC_F64_SLOTS doubles followed by GGNN_METRIC_I64_SLOTS int64, one DEVICE allocation, zeroed by the caller
 * when a sum starts.  workspace: GGNN_METRIC_WS_WORDS 8-byte words of DEVICE memory, zero before the first call (the call
 * leaves its last word zero again); one per stream that may have a launch in flight.
 * GGNN_METRIC_BLOCKS workgroups each walk a fixed share of the elements; their partial sums go through the workspace and the
 * last workgroup to arrive (an integer ticket) adds them in index order INTO acc: no floating-point atomics, the same bits
 * on every run, on any stream and from a replayed hipGraph (replays keep adding).
 * GGNN_EINVAL without a launch: args / acc / workspace NULL, n_terms outside 0..4, n_thr outside 0..16, a negative count,
 * a missing operand of a non-empty term, an unknown mode. */
#define GGNN_METRIC_MAX_TERMS 4
#define GGNN_METRIC_MAX_THR 16
#define GGNN_METRIC_BLOCKS 64
#define GGNN_METRIC_F64_SLOTS 9  /* err[4] | norm[4] | loss */
#define GGNN_METRIC_I64_SLOTS 49 /* TP[16] | FP[16] | FN[16] | batches */
#define GGNN_METRIC_WS_WORDS (GGNN_METRIC_BLOCKS * 56 + 1) /* per workgroup 8 doubles | 48 int64; + the arrival counter */
#define GGNN_METRIC_CLASSIFIER 0
#define GGNN_METRIC_REGRESSOR 1
typedef struct ggnn_metric_args {
  const float* pred[GGNN_METRIC_MAX_TERMS];
  const float* target[GGNN_METRIC_MAX_TERMS];
  const float* mask[GGNN_METRIC_MAX_TERMS];
  int64_t n_rows[GGNN_METRIC_MAX_TERMS];
  int64_t ld[GGNN_METRIC_MAX_TERMS];      /* row stride of pred and target, in floats */
  int64_t ld_mask[GGNN_METRIC_MAX_TERMS]; /* row stride of mask */
  int32_t col[GGNN_METRIC_MAX_TERMS];
  const float* score;
  const int64_t* label;
  const float* label_mask; /* GGNN_METRIC_REGRESSOR only */
  int64_t n;
  int64_t ld_label_mask;
  float thr[GGNN_METRIC_MAX_THR];
  const float* loss; /* optional, DEVICE [1] */
  void* acc;
  void* workspace;
  int32_t n_terms, n_thr, mode, with_norm;
} ggnn_metric_args;
int ggnn_metric_record(const ggnn_metric_args* args, ggnn_stream_t stream);

/* Bytes of device scratch one model forward needs (projections + aggregates + h/c), so a
 * caller can size a single arena; the Python host allocates the same amounts as tensors. */
size_t ggnn_workspace_bytes(int64_t n_grain, int64_t n_joint, int64_t E);

#ifdef __cplusplus
}
#endif
#endif /* GGNN_H_ */
