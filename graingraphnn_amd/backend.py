"""Thin tensor-level wrapper over the C ABI (include/ggnn.h).  One method per entry point;
tensors in, launches enqueued on the current HIP stream, nothing returned but the outputs
written in place.  `HipBackend` is the only backend the package ships: it refuses CPU
tensors and raises if libggnn.so cannot be loaded -- there is no CPU fallback."""
import ctypes
import os

import torch

from . import _lib
from ._lib import (AggregateArgs, AggregateBwdArgs, AggregateEncArgs, DecCellArgs, EncCellArgs, EncValuesArgs, EpilogueArgs, PrepareEdge, ProjectArgs,
                   RefreshEdge, check, ptr)



class CSR:
    """Destination-grouped edge list of one edge type (all int32, device resident)."""
    __slots__ = ("rowptr", "col", "perm", "row", "unit_ptr", "units", "E", "E_dev")

    def __init__(self, rowptr, col, perm, row, unit_ptr, units, E, E_dev=None):
        self.rowptr, self.col, self.perm, self.row = rowptr, col, perm, row
        self.unit_ptr, self.units, self.E = unit_ptr, units, E
        # int64 [1] on the device or None: the number of edges the per-edge kernels read at RUN time (tables that are
        # rebuilt in place under captured launches: GrainRollout's event loop; include/ggnn.h, ggnn_prepare_edge.E_dev)
        self.E_dev = E_dev


class _WordArena:
    """Hands out int32 tables one behind the other, each starting on a 16-byte boundary; without a buffer it only counts."""

    def __init__(self, buf=None):
        self.buf, self.at = buf, 0

    def take(self, n):
        t = None if self.buf is None else self.buf[self.at:self.at + n]
        self.at += (n + 3) & ~3
        return t


def _csr_tables(lib, take, E_cap, n_src, n_dst, args=None):
    """The tables of one list with up to E_cap edges, each from `take(n int32 words)`, in the one order and with the sizes
    everything else relies on: -> (rowptr, col, perm, row, unit_ptr, units [n_units, 8], flags, workspace), their addresses
    written into `args` (a CsrArgs; edge_index and E are the caller's).  args=None: `take` only counts, nothing is returned."""
    E_cap, n_dst = int(E_cap), int(n_dst)
    n_e, n_units = max(E_cap, 1), lib.ggnn_csr_max_units(E_cap, n_dst)
    nbytes = lib.ggnn_csr_workspace_bytes(E_cap, n_dst)   # (sized for the capacity: enough for any shorter list)
    rowptr, col, perm, row, unit_ptr, units, flags, ws = [
        take(n) for n in (n_dst + 1, n_e, n_e, n_e, n_dst + 1, 8 * n_units, 2, nbytes // 4 + 1)]
    if args is None:
        return None
    a = args
    a.n_src, a.n_dst = n_src, n_dst
    a.rowptr, a.col, a.perm, a.row = rowptr.data_ptr(), col.data_ptr(), perm.data_ptr(), row.data_ptr()
    a.unit_ptr, a.units, a.flags = unit_ptr.data_ptr(), units.data_ptr(), flags.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    return rowptr, col, perm, row, unit_ptr, units.view(n_units, 8), flags, ws


class CsrInPlace:
    """See HipBackend.csr_in_place."""

    def __init__(self, backend, shapes, device, masks=None, unions=None):
        if not 1 <= len(shapes) <= 4:
            raise _lib.GGNNError("csr_in_place: one to four lists")
        self.be, self.shapes = backend, [tuple(int(v) for v in s) for s in shapes]
        # masked lists (ggnn_csr_mask): refilled with the same mask; their tables' edge count lives in a device word
        self.masks, self.kept = _csr_masks(masks, len(self.shapes), device)
        # a disjoint union (ggnn_csr_union): the masks' indices are local ones, every refill (the offset tensors are kept)
        self.unions, self._union_tensors = _csr_unions(unions, len(self.shapes))
        words = sum(backend.csr_arena_words(cap, n_dst) for cap, _, n_dst in self.shapes)
        arena = _WordArena(torch.empty(words, dtype=torch.int32, device=device))
        self.args = (_lib.CsrArgs * len(self.shapes))()
        self.csr = [CSR(*_csr_tables(backend.lib, arena.take, cap, n_src, n_dst, a)[:6], 0)
                    for a, (cap, n_src, n_dst) in zip(self.args, self.shapes)]

    def rebuild(self, lists):
        """-> the CSR objects; those of masked lists carry E_dev = their kept-edge word."""
        for a, csr, ei, (cap, _, _) in zip(self.args, self.csr, lists, self.shapes):
            if ei.dtype != torch.int64 or ei.dim() != 2 or ei.size(0) != 2 or not ei.is_contiguous() or not ei.is_cuda:
                raise _lib.GGNNError("edge_index must be a contiguous int64 [2, E] device tensor")
            E = ei.size(1)
            if E > cap:
                raise _lib.GGNNError("csr_in_place: a list grew beyond its capacity")
            a.edge_index, a.E = ei.data_ptr(), E
            csr.E = E
        for csr, w in zip(self.csr, self.kept):
            if w is not None:
                csr.E_dev = w
        _build_csr(self.be.lib, self.args, self.masks, self.unions, len(self.shapes))
        return self.csr


def _csr_masks(masks, n, device):
    """[(skip_src, skip_dst) or None] -> (ctypes array of CsrMask, [int64 [1] kept-edge word or None]); (None, [None] * n)
    when nothing is masked."""
    if masks is None or all(m is None or tuple(m) == (-1, -1) for m in masks):
        return None, [None] * n
    if len(masks) != n:
        raise _lib.GGNNError("one mask per list")
    arr, kept = (_lib.CsrMask * n)(), []
    for a, m in zip(arr, masks):
        s, d = (-1, -1) if m is None else (int(m[0]), int(m[1]))
        if s < -1 or d < -1:
            raise _lib.GGNNError("skip_src / skip_dst: a node index or -1")
        w = torch.zeros(1, dtype=torch.int64, device=device) if (s, d) != (-1, -1) else None
        a.skip_src, a.skip_dst, a.E_kept = s, d, (w.data_ptr() if w is not None else None)
        kept.append(w)
    return arr, kept


def _csr_unions(unions, n):
    """[(src_off, dst_off) or None], each offset an int64 [n_traj + 1] device tensor or None -> (ctypes array of CsrUnion,
    the tensors it points into); (None, ()) when no list is split."""
    if unions is None or all(u is None or (u[0] is None and u[1] is None) for u in unions):
        return None, ()
    if len(unions) != n:
        raise _lib.GGNNError("one union per list")
    arr, keep = (_lib.CsrUnion * n)(), []
    for a, u in zip(arr, unions):
        offs = [t for t in (u or ()) if t is not None]
        if offs:
            a.src_off, a.dst_off, a.n_traj = ptr(u[0]), ptr(u[1]), _offsets(offs, "union offsets")
            keep += offs
    return arr, tuple(keep)


def _build_csr(lib, args, masks, unions, n):
    """ggnn_build_csr_batch, or -- lists of a disjoint union -- ggnn_build_csr_batch_traj."""
    if unions is None:
        _lib.check(lib.ggnn_build_csr_batch(args, masks, n, _lib.current_stream()), "ggnn_build_csr_batch")
    else:
        _lib.check(lib.ggnn_build_csr_batch_traj(args, masks, unions, n, _lib.current_stream()), "ggnn_build_csr_batch_traj")


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.GGNNError(
                "graingraphnn_amd runs on MI355X only: got a CPU tensor (no CPU fallback exists; "
                "move the model and the graph to 'cuda')")


def _f32c(t, name):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise _lib.GGNNError(f"{name} must be a contiguous float32 tensor")
    return t


def _offsets(tensors, name, entries=None):
    """The offsets of a disjoint union (csrc/segments.h): contiguous int64 [n_traj + 1] device tensors, n_traj >= 1, all of
    one length -- of `entries` where the caller knows how many there must be; -> n_traj."""
    want = tensors[0].numel() if entries is None else entries
    for t in tensors:
        if not t.is_cuda or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous() or t.numel() < 2 or t.numel() != want:
            raise _lib.GGNNError(f"{name} must be contiguous int64 [n_traj + 1] on the device, of one length")
    return want - 1


def _check_einfo(einfo, E):
    if einfo.dtype != torch.float32 or not einfo.is_contiguous() or einfo.dim() != 2 \
            or einfo.size(1) != _lib.GGNN_EINFO_ROW or einfo.size(0) < E + _lib.GGNN_UNIT_EDGES:
        raise _lib.GGNNError("einfo must be contiguous float32 [E + GGNN_UNIT_EDGES, GGNN_EINFO_ROW]")


def _prepare_edges(items):
    """-> the ggnn_prepare_edge array of edge_prepare's items."""
    arr = (PrepareEdge * max(len(items), 1))()
    for a, (csr, ea, xs, xd, einfo) in zip(arr, items):
        _require_cuda(csr.col, ea, xs, xd, einfo)
        if einfo.size(0) < ea.numel() + _lib.GGNN_UNIT_EDGES or einfo.size(1) != _lib.GGNN_EINFO_ROW:
            raise _lib.GGNNError("einfo must be [E + GGNN_UNIT_EDGES, GGNN_EINFO_ROW]")
        a.col, a.perm, a.row = csr.col.data_ptr(), csr.perm.data_ptr(), csr.row.data_ptr()
        a.edge_attr, a.x_src, a.x_dst = ea.data_ptr(), xs.data_ptr(), xd.data_ptr()
        a.einfo = einfo.data_ptr()
        a.ldx_src, a.ldx_dst, a.E, a.f_src = xs.stride(0), xd.stride(0), ea.numel(), xs.size(1)
        a.E_dev = ptr(csr.E_dev)   # (a topology that shrinks in place under captured launches)
    return arr


class HipBackend:
    name = "hip"
    FUSED_DECODER_MIN_JOINTS = 6000

    def __init__(self):
        self.lib = _lib.load()
        self._tape = None  # while a list: every hot-path launch is also recorded as (cfunc, name, cargs)
        self._range_flags = {}  # device -> int32 word the fp16 two-piece kernels report clamped activations in
        self._rowgemm_ws = {}   # (device, stream, bytes) -> weight-plane workspace of ggnn_rowgemm
        self._mse_ws = {}       # (device, stream) -> partial sums + arrival counter of ggnn_masked_mse
        self._metric_ws = {}    # (device, stream) -> partial rows + arrival counter of ggnn_metric_record
        # encoder cell as ONE fused sweep + gate GEMM launch (ggnn_encoder_cell_batch; bf16x6 arithmetic
        # only).  GGNN_ENC=split keeps the sweep and the gate GEMM as separate launches (development).
        self.fused_encoder = (self.lib.ggnn_gemm_mode() == 1 and os.environ.get("GGNN_ENC", "") != "split")
        # The decoder cell of a model: ONE kernel (ggnn_decoder_cell_batch, the default with the bf16 / fp16 matrix-core
        # GEMM mode) or projection + sweeps + gate GEMM (GGNN_DEC=split; always under GGNN_GEMM=fp32).
        # GGNN_DEC=fused-classifier / fused-regressor: the fused cell for that model only (development).
        # By default (GGNN_DEC unset) the plan follows the graph's size (engine.run_cells): a fused cell is one dependent
        # chain of ~110 us per 16-node tile however few tiles there are, so below FUSED_DECODER_MIN_JOINTS junctions the
        # three short kernels win (1 043-grain fixture: 8 080 vs 5 620 steps/s; 64 x 118 grains batched: 205 k vs 220 k
        # trajectory-steps/s; 10 000 grains: 2 380 vs 2 920 steps/s).  GGNN_DEC=fused: the fused cell whatever the size.
        dec = os.environ.get("GGNN_DEC", "auto")
        self.fused_decoder = False
        self.fused_decoder_min_joints = 0
        if self.lib.ggnn_gemm_mode() == 1 and (dec == "auto" or dec.startswith("fused")):
            self.fused_decoder = {"auto": True, "fused": True, "fused-classifier": "classifier",
                                  "fused-regressor": "regressor"}.get(dec, False)
            if dec == "auto":
                self.fused_decoder_min_joints = int(os.environ.get("GGNN_DEC_MIN_JOINTS", str(self.FUSED_DECODER_MIN_JOINTS)))

        # the fused decoder plan's value rows as [blocks][N][96] (GGNN_OUT_BLOCK_MAJOR: every workgroup of the projection
        # stores contiguous runs, and a (edge type, gate) pass of the cell gathers from one dense [N, 96] matrix --
        # dec_cell_kernel 110.2 -> 105.5 us, project_x6_kernel 22.8 -> 21.9 us per launch, 3 020 -> 3 054 steps/s on one box,
        # profiles/r6_value_rows_layout.txt); GGNN_VLAYOUT=rows: [N, ncols] (A/B runs)
        self.value_rows_block_major = os.environ.get("GGNN_VLAYOUT", "block") != "rows"
        # the fused decoder plan's value rows written by the ENCODER cell of the same model, behind its LSTM update
        # (ggnn_encoder_cell_values_batch; engine.value_epilogues decides where it applies): one launch and one dependent
        # stage less per model, and no re-read of x | h1.  GGNN_ENC_VALUES=0 keeps the separate projection (A/B runs).
        # With the decoder plan left to the graph's size (GGNN_DEC unset) the epilogue goes wherever the fused decoder does;
        # a forced decoder plan (GGNN_DEC=fused...: development, the decoder cell alone) keeps the projection launch below
        # FUSED_DECODER_MIN_JOINTS junctions, as the plan around the cell was before.
        self.encoder_values = os.environ.get("GGNN_ENC_VALUES", "1") != "0"
        self.encoder_values_min_joints = 0 if dec == "auto" else self.FUSED_DECODER_MIN_JOINTS

    def f16_projection(self) -> bool:
        """The fused decoder plan's value projection in the cells' three-product arithmetic (GGNN_PRECISION_F16X2) when the
        packed weights allow; GGNN_PROJ=x6 keeps the six-product split (development, A/B runs)."""
        return os.environ.get("GGNN_PROJ", "") != "x6"

    # -- launch tape: the drop-in forward() issues the same dozen launches with the same arguments
    # step after step (test.py:382-383); re-issuing the recorded C calls skips the per-launch
    # Python work (argument checks, ctypes struct filling), which otherwise outweighs the kernels.
    def _launch(self, fn, name, *cargs):
        check(fn(*cargs), name)
        if self._tape is not None:
            self._tape.append((fn, name, cargs))

    def start_tape(self):
        self._tape = []

    def stop_tape(self):
        tape, self._tape = self._tape, None
        return tape

    @staticmethod
    def replay(tape):
        for fn, name, cargs in tape:
            rc = fn(*cargs)
            if rc:
                check(rc, name)

    # -- CSR ---------------------------------------------------------------------------
    def build_csr(self, edge_index, n_src, n_dst):
        """edge_index [2, E] int64 (cuda) -> CSR.  Raises IndexError on out-of-range indices
        (one host sync, only when a topology is first seen)."""
        return self.build_csr_batch([(edge_index, n_src, n_dst)])[0]

    def csr_arena_words(self, E_cap, n_dst):
        """int32 words of one list's tables (row pointers, columns, permutation, rows, unit tables, flags, workspace) for up
        to E_cap edges, every table starting on a 16-byte boundary."""
        count = _WordArena()
        _csr_tables(self.lib, count.take, E_cap, 0, n_dst)
        return count.at

    def csr_in_place(self, shapes, device, masks=None, unions=None):
        """Tables that are rebuilt in place: `shapes` = [(E_cap, n_src, n_dst)] (at most four lists) -> a CsrInPlace whose
        `rebuild([edge_index [2, E <= E_cap]])` fills the SAME device tables for the new lists (unchecked: validated lists)
        and returns the same CSR objects with their E updated -- tensors of capacity size, addresses that never change, so
        launches captured on an earlier, longer version of a list keep reading valid tables.  masks / unions: as in
        build_csr_batch, applied at every refill."""
        return CsrInPlace(self, shapes, device, masks, unions)

    def build_csr_batch(self, lists, check=True, masks=None, unions=None):
        """[(edge_index [2, E] int64 cuda, n_src, n_dst)] -> [CSR]: ggnn_build_csr_batch, up to four lists per sequence of
        launches (engine.GraphCSR builds the three edge types of a topology in one; a topological event rebuilds them),
        one range check = one host synchronisation behind the last (`check=False`: lists the caller has validated -- the
        kernels skip an out-of-range edge either way --: no read-back, the host goes on enqueueing).  (Tables that are
        refilled IN PLACE per event: `csr_in_place`.)  masks: None, or per list None / (skip_src, skip_dst) -- the tables of
        the list without the edges from skip_src / into skip_dst (ggnn_csr_mask); the CSR of a masked list has
        E = the list's length and E_dev = the number of edges it kept (device word).  unions: None, or per list None /
        (src_off, dst_off) -- the lists of a disjoint union of trajectories, int64 [n_traj + 1] device offsets of the
        source / destination node type or None (that side is not split): the list's mask then skips LOCAL indices
        (ggnn_csr_union, ggnn_build_csr_batch_traj)."""
        out, todo = [], list(lists)
        mtodo = list(masks) if masks is not None else [None] * len(todo)
        utodo = list(unions) if unions is not None else [None] * len(todo)
        while todo:
            chunk, todo = todo[:4], todo[4:]
            mchunk, mtodo = mtodo[:4], mtodo[4:]
            uchunk, utodo = utodo[:4], utodo[4:]
            marr, kept = _csr_masks(mchunk, len(chunk), chunk[0][0].device)
            uarr, _ = _csr_unions(uchunk, len(chunk))
            arr = (_lib.CsrArgs * len(chunk))()
            keep = []
            arena = None
            if not check:
                # unchecked builds run once per topological event: every table of the chunk out of ONE allocation (two
                # dozen allocator calls and six fills otherwise; the unit table's unused tail and the range flags that
                # nobody reads stay uninitialised)
                need = sum(self.csr_arena_words(int(ei_.size(1)), n_dst) for ei_, _, n_dst in chunk)
                arena = _WordArena(torch.empty(need, dtype=torch.int32, device=chunk[0][0].device))
            for a, (edge_index, n_src, n_dst) in zip(arr, chunk):
                _require_cuda(edge_index)
                if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
                    raise _lib.GGNNError("edge_index must be int64 [2, E]")
                ei = edge_index.contiguous()
                E, dev = ei.size(1), ei.device
                take = arena.take if arena is not None else (lambda n: torch.empty(n, dtype=torch.int32, device=dev))
                *tables, flags, ws = _csr_tables(self.lib, take, E, n_src, n_dst, a)
                if arena is None:   # (a checked build: the flags are read back, the unit table is defined to its end)
                    tables[-1].zero_()
                    flags.zero_()
                a.edge_index, a.E = ei.data_ptr(), E
                keep.append((ei, ws, flags, n_src, n_dst))
                out.append(CSR(*tables, E, kept[len(keep) - 1]))
            _build_csr(self.lib, arr, marr, uarr, len(chunk))
            if not check:   # (ei / ws / flags are only used by launches on this stream: the allocator keeps them until those ran)
                continue
            bad = torch.stack([k[2][0] for k in keep]).cpu()   # (the synchronisation; also keeps ei / ws alive until here)
            for k, f in zip(keep, bad.tolist()):
                if f & 1:
                    raise IndexError(f"edge_index has entries outside [0,{k[3]}) x [0,{k[4]})")
        return out

    # -- per-edge geometry -------------------------------------------------------------
    def edge_prepare(self, items):
        """items: list of (csr, edge_attr [E] COO order, x_src, x_dst, einfo_out [E + 3, GGNN_EINFO_ROW])."""
        arr = _prepare_edges(items)
        self._launch(self.lib.ggnn_edge_prepare, "ggnn_edge_prepare", arr, len(items), _lib.current_stream())

    # -- projection --------------------------------------------------------------------
    def project(self, x, F, h, wp, bp, out):
        self.project_batch([(x, F, h, wp, bp, out)])

    def project_batch(self, problems):
        """Up to four projections in one launch (ggnn_project_batch); each item: (x, F, h, wp, bp, out[, precision]).
        All with h or all without."""
        arr = (ProjectArgs * len(problems))()
        if len({pr[2] is None for pr in problems}) > 1:
            raise _lib.GGNNError("ggnn_project_batch: every problem with a hidden state or none of them "
                                 "(problems with k2 = 96 and k2 = 0 cannot share a launch)")
        for a, (x, F, h, wp, bp, out, *rest) in zip(arr, problems):
            a.precision = rest[0] if rest else 0   # optional 7th element: _lib.GGNN_PRECISION_BF16 (training, autocast)
            _require_cuda(x, h, wp, bp, out)
            # what the C side cannot see behind a raw pointer: dtypes, unit column strides, the weight's shape
            k2 = 0 if h is None else h.size(1)
            for t, name in ((x, "x"), (h, "h"), (wp, "wp"), (bp, "bp"), (out, "out")):
                if t is not None and t.dtype != torch.float32:
                    raise _lib.GGNNError(f"ggnn_project_batch: {name} must be float32")
            if x.dim() != 2 or x.stride(1) != 1 or x.size(1) < F or out.dim() != 2 or out.stride(1) != 1:
                raise _lib.GGNNError("ggnn_project_batch: x [M, >= F] and out [M, ncols] need unit column stride")
            if h is not None and (h.dim() != 2 or h.stride(1) != 1 or h.size(0) != x.size(0)):
                raise _lib.GGNNError("ggnn_project_batch: h must be [M, k2] with unit column stride")
            if not wp.is_contiguous() or wp.dim() != 2 or wp.size(1) != ((F + 3) & ~3) + k2:
                raise _lib.GGNNError(f"ggnn_project_batch: wp must be contiguous [ncols, roundup4(F) + k2] = "
                                     f"[*, {((F + 3) & ~3) + k2}], got {tuple(wp.shape)}")
            if bp.numel() != wp.size(0) or not bp.is_contiguous():
                raise _lib.GGNNError("ggnn_project_batch: bp must hold ncols contiguous values")
            if out.size(0) != x.size(0) or out.size(1) < wp.size(0):
                raise _lib.GGNNError("ggnn_project_batch: out must be [M, >= ncols]")
            a.X, a.Wp, a.bias, a.out = x.data_ptr(), wp.data_ptr(), bp.data_ptr(), out.data_ptr()
            a.H = None if h is None else h.data_ptr()
            a.ldx, a.ldh, a.M, a.ldo = x.stride(0), 0 if h is None else h.stride(0), x.size(0), out.stride(0)
            a.F, a.k2, a.ncols = F, 0 if h is None else h.size(1), wp.size(0)
        self._launch(self.lib.ggnn_project_batch, "ggnn_project_batch", arr, len(problems), _lib.current_stream())

    # -- aggregation -------------------------------------------------------------------
    @staticmethod
    def _sweep_args(a, csr, einfo, p_src, p_dst, h_src, ep, agg, v_off, u_off, u4_off, a_off,
                    a_gstride, sc_off, n_gates, pad_n=0):
        _require_cuda(csr.unit_ptr, einfo, p_src, p_dst, h_src, ep, agg)
        a.unit_ptr, a.units, a.einfo = csr.unit_ptr.data_ptr(), csr.units.data_ptr(), einfo.data_ptr()
        a.p_src, a.p_dst = p_src.data_ptr(), p_dst.data_ptr()
        a.h_src = None if h_src is None else h_src.data_ptr()
        a.edge_params, a.agg = ep.data_ptr(), agg.data_ptr()
        a.ldp_src, a.ldp_dst, a.ld_agg = p_src.stride(0), p_dst.stride(0), agg.stride(0)
        a.ldh_src = 0 if h_src is None else h_src.stride(0)
        a.n_src, a.n_dst, a.E = p_src.size(0), p_dst.size(0), csr.E
        a.v_off, a.u_off, a.u4_off, a.a_off, a.a_gstride, a.sc_off, a.n_gates = (
            v_off, u_off, u4_off, a_off, a_gstride, sc_off, n_gates)
        a.pad_n = pad_n

    def aggregate(self, *sweep):
        """One sweep (include/ggnn.h, ggnn_aggregate_args): (csr, einfo, p_src, p_dst, h_src,
        ep, agg, v_off, u_off, u4_off, a_off, a_gstride, sc_off, n_gates[, pad_n]).  h_src: the source node
        type's hidden state [n_src, 96] or None (encoder); pad_n: columns behind the sweep's scalars that it zeroes in
        every gate row (the training path's padded gate rows)."""
        self.aggregate_batch([sweep])

    def aggregate_batch(self, sweeps):
        """The 1..3 sweeps of one cell in one launch (ggnn_period_gat_aggregate_batch); each item
        is the argument tuple of `aggregate`."""
        arr = (AggregateArgs * len(sweeps))()
        for a, sweep in zip(arr, sweeps):
            self._sweep_args(a, *sweep)
        self._launch(self.lib.ggnn_period_gat_aggregate_batch, "ggnn_period_gat_aggregate_batch", arr,
                     len(sweeps), _lib.current_stream())

    def aggregate_enc_batch(self, sweeps):
        """Encoder sweeps (h = 0) with the edge values on the matrix cores
        (ggnn_period_gat_aggregate_enc_batch); each item: (csr, einfo, p_dst, wv_frag, agg, u4_off, a_off,
        a_gstride, sc_off, n_gates)."""
        arr = (AggregateEncArgs * len(sweeps))()
        for a, (csr, einfo, p_dst, wvf, agg, u4_off, a_off, a_gstride, sc_off, n_gates) in zip(arr, sweeps):
            _require_cuda(csr.unit_ptr, einfo, p_dst, wvf, agg)
            if wvf.dtype != torch.float32 or wvf.numel() != 6 * n_gates * 3 * 64:
                raise _lib.GGNNError("wv_frag does not match n_gates (see packing.value_fragments)")
            a.unit_ptr, a.units, a.einfo = csr.unit_ptr.data_ptr(), csr.units.data_ptr(), einfo.data_ptr()
            a.p_dst, a.wv_frag, a.agg = p_dst.data_ptr(), wvf.data_ptr(), agg.data_ptr()
            a.ldp_dst, a.ld_agg, a.n_dst, a.E = p_dst.stride(0), agg.stride(0), p_dst.size(0), csr.E
            a.u4_off, a.a_off, a.a_gstride, a.sc_off, a.n_gates = u4_off, a_off, a_gstride, sc_off, n_gates
        self._launch(self.lib.ggnn_period_gat_aggregate_enc_batch, "ggnn_period_gat_aggregate_enc_batch", arr,
                     len(sweeps), _lib.current_stream())

    def encoder_cell_batch(self, problems):
        """ggnn_encoder_cell_batch (include/ggnn.h): the encoder cell (h = c = 0) of up to four (model, destination
        node type) problems in one launch.  Each item: (sweeps, x_dst, wstream, w2_tail, h_out, c_out) with sweeps =
        [(csr, einfo)] for the 1 or 2 incoming edge types; wstream / w2_tail: packing.encoder_cell_stream."""
        arr = (EncCellArgs * len(problems))()
        for a, prob in zip(arr, problems):
            self._enc_cell_args(a, prob)
        self._launch(self.lib.ggnn_encoder_cell_batch, "ggnn_encoder_cell_batch", arr, len(problems),
                     _lib.current_stream())

    def encoder_cell_values_batch(self, problems):
        """ggnn_encoder_cell_values_batch (include/ggnn.h): encoder_cell_batch's problems, each with the decoder's value
        rows of its node type as an epilogue.  Each item: (cell problem as for encoder_cell_batch, vstream, v_out) with
        vstream = packing.encoder_values_stream (int16 [4 n_blocks, GGNN_DC_SLICE_BYTES / 2]) and v_out the projection
        buffer the decoder cell reads block-major: its first n_blocks 96 n_dst floats are [n_blocks][n_dst][96]."""
        arr = (EncValuesArgs * len(problems))()
        for a, (prob, vstream, v_out) in zip(arr, problems):
            self._enc_cell_args(a.cell, prob)
            _require_cuda(vstream, v_out)
            n = prob[1].size(0)
            nslices = vstream.numel() * 2 // _lib.GGNN_DC_SLICE_BYTES
            if vstream.dtype != torch.int16 or not vstream.is_contiguous() or nslices % 4 \
                    or vstream.numel() * 2 != nslices * _lib.GGNN_DC_SLICE_BYTES \
                    or not 1 <= nslices // 4 <= _lib.GGNN_ENC_VALUES_MAX_BLOCKS:
                raise _lib.GGNNError("ggnn_encoder_cell_values_batch: vstream is not packing.encoder_values_stream")
            nb = nslices // 4
            if v_out.dtype != torch.float32 or not v_out.is_contiguous() or v_out.numel() < nb * n * 96:
                raise _lib.GGNNError(f"ggnn_encoder_cell_values_batch: v_out must be contiguous float32 with at least "
                                     f"{nb} x {n} x 96 elements")
            a.vstream, a.v_out, a.n_blocks = vstream.data_ptr(), v_out.data_ptr(), nb
        self._launch(self.lib.ggnn_encoder_cell_values_batch, "ggnn_encoder_cell_values_batch", arr, len(problems),
                     _lib.current_stream())

    def _enc_cell_args(self, a, problem):
        """Fill one ggnn_enc_cell_args from an encoder_cell_batch item (checked)."""
        sweeps, x_dst, wstream, w2_tail, h_out, c_out, *rest = problem
        _require_cuda(x_dst, wstream, w2_tail, h_out, c_out)
        n, n_in = x_dst.size(0), len(sweeps)
        for t, name in ((x_dst, "x_dst"), (h_out, "h_out"), (c_out, "c_out"), (w2_tail, "w2_tail")):
            if t.dtype != torch.float32 or t.dim() < 2 or t.stride(-1) != 1:
                raise _lib.GGNNError(f"ggnn_encoder_cell_batch: {name} must be float32 with unit column stride")
        if n_in not in (1, 2) or tuple(h_out.shape) != (n, 96) or not h_out.is_contiguous() \
                or tuple(c_out.shape) != (n, 96) or not c_out.is_contiguous():
            raise _lib.GGNNError("ggnn_encoder_cell_batch: h_out / c_out must be contiguous [n_dst, 96], 1 or 2 "
                                 "incoming edge types")
        if wstream.dtype != torch.int16 or not wstream.is_contiguous() \
                or wstream.numel() * 2 != 3 * (4 * n_in + 1) * _lib.GGNN_DC_SLICE_BYTES:
            raise _lib.GGNNError("ggnn_encoder_cell_batch: wstream is not packing.encoder_cell_stream of this "
                                 "number of incoming edge types")
        if tuple(w2_tail.shape) != (3, n_in, 6, 64) or not w2_tail.is_contiguous():
            raise _lib.GGNNError("ggnn_encoder_cell_batch: w2_tail must be contiguous [3, n_in, 6, 64]")
        for sw, (csr, einfo) in zip(a.sweeps, sweeps):
            _require_cuda(csr.rowptr, einfo)
            if csr.rowptr.numel() != n + 1:
                raise _lib.GGNNError("the sweep's CSR does not have one row per destination node")
            _check_einfo(einfo, csr.E)
            sw.rowptr, sw.einfo, sw.E = csr.rowptr.data_ptr(), einfo.data_ptr(), csr.E
        a.x_dst, a.h_out, a.c_out = x_dst.data_ptr(), h_out.data_ptr(), c_out.data_ptr()
        a.wstream, a.w2_tail = wstream.data_ptr(), w2_tail.data_ptr()
        # (optional last element of a problem: the caller's own flag word -- a rollout's -- instead of the device-wide one)
        a.flags = (rest[0] if rest and rest[0] is not None else self.range_flag(x_dst.device)).data_ptr()
        a.n_dst, a.ldx, a.n_in, a.f_dst = n, x_dst.stride(0), n_in, x_dst.size(1)

    def range_flag(self, device):
        """The device word the two-piece fp16 kernels OR GGNN_FLAG_F16_RANGE into when they clamp an activation
        (include/ggnn.h, OPERAND RANGE); one per device, never cleared by the kernels."""
        key = torch.device(device)
        if key.index is None:
            key = torch.device(key.type, torch.cuda.current_device())
        flag = self._range_flags.get(key)
        if flag is None:
            flag = self._range_flags[key] = torch.zeros(1, dtype=torch.int32, device=key)
        return flag

    def range_exceeded(self, device="cuda", clear=True, flag=None) -> bool:
        """True when a fused cell has clamped an activation to fp16's range since the flag was last cleared: its
        results are then NOT the reference's (re-run with GGNN_DEC=split / GGNN_ENC=split, whose bf16 x 3 split
        covers fp32's range).  One host sync.  `flag`: a caller's own word (GrainRollout keeps one per rollout, so that
        two rollouts on a device do not consume each other's reports); default: the device-wide word."""
        flag = self.range_flag(device) if flag is None else flag
        hit = bool(int(flag.item()) & _lib.GGNN_FLAG_F16_RANGE)
        if hit and clear:
            flag.zero_()
        return hit

    def decoder_cell_batch(self, problems):
        """ggnn_decoder_cell_batch (include/ggnn.h): the decoder cell of up to four (model, destination node type)
        problems in one launch.  Each item: (sweeps, x_dst, h_dst, c_in, wstream, w2_tail, h_out, c_out) with
        sweeps = [(csr, einfo, h_src, v_src, v_off, edge_params)] for the 1 or 2 incoming edge types; wstream /
        w2_tail: packing.decoder_cell_stream."""
        arr = (DecCellArgs * len(problems))()
        for a, (sweeps, x_dst, h_dst, c_in, wstream, w2_tail, h_out, c_out, *rest) in zip(arr, problems):
            _require_cuda(x_dst, h_dst, c_in, wstream, w2_tail, h_out, c_out)
            n, n_in = x_dst.size(0), len(sweeps)
            for t, name in ((x_dst, "x_dst"), (h_dst, "h_dst"), (c_in, "c_in"), (h_out, "h_out"), (c_out, "c_out"),
                            (w2_tail, "w2_tail")):
                if t.dtype != torch.float32 or t.dim() < 2 or t.stride(-1) != 1:
                    raise _lib.GGNNError(f"ggnn_decoder_cell_batch: {name} must be float32 with unit column stride")
            if n_in not in (1, 2) or tuple(h_dst.shape) != (n, 96) or tuple(c_in.shape) != (n, 96) \
                    or not c_in.is_contiguous() or tuple(h_out.shape) != (n, 96) or not h_out.is_contiguous() \
                    or tuple(c_out.shape) != (n, 96) or not c_out.is_contiguous():
                raise _lib.GGNNError("ggnn_decoder_cell_batch: h_dst / c_in / h_out / c_out must be [n_dst, 96] "
                                     "(c_in, h_out, c_out contiguous), 1 or 2 incoming edge types")
            if wstream.dtype != torch.int16 or not wstream.is_contiguous() \
                    or wstream.numel() * 2 != 4 * (7 * n_in + 4) * _lib.GGNN_DC_SLICE_BYTES:
                raise _lib.GGNNError("ggnn_decoder_cell_batch: wstream is not packing.decoder_cell_stream of this "
                                     "number of incoming edge types")
            if tuple(w2_tail.shape) != (4, n_in, 6, 64) or not w2_tail.is_contiguous():
                raise _lib.GGNNError("ggnn_decoder_cell_batch: w2_tail must be contiguous [4, n_in, 6, 64]")
            for sw, (csr, einfo, h_src, v_src, v_off, ep, *v_bm) in zip(a.sweeps, sweeps):
                v_bm = bool(v_bm and v_bm[0])   # optional 7th element: v_src is GGNN_OUT_BLOCK_MAJOR ([blocks][n_src][96])
                _require_cuda(csr.rowptr, csr.col, einfo, h_src, v_src, ep)
                if csr.rowptr.numel() != n + 1:
                    raise _lib.GGNNError("the sweep's CSR does not have one row per destination node")
                _check_einfo(einfo, csr.E)
                for t, name in ((h_src, "h_src"), (v_src, "v_src")):
                    if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.size(0) != h_src.size(0):
                        raise _lib.GGNNError(f"ggnn_decoder_cell_batch: {name} must be float32 [n_src, *] with unit "
                                             "column stride")
                if v_bm and (not v_src.is_contiguous() or v_off % 96):
                    raise _lib.GGNNError("ggnn_decoder_cell_batch: block-major value rows live in a contiguous buffer, "
                                         "v_off a multiple of 96")
                if h_src.size(1) < 96 or v_off < 0 or v_off + 4 * 96 > v_src.size(1):
                    raise _lib.GGNNError("ggnn_decoder_cell_batch: h_src needs 96 columns, the four gates' value rows "
                                         "must lie inside a v_src row")
                if ep.dtype != torch.float32 or not ep.is_contiguous() or tuple(ep.shape) != (4, 3, 96):
                    raise _lib.GGNNError("edge_params must be contiguous float32 [4, 3, 96]")
                sw.rowptr, sw.col, sw.einfo = csr.rowptr.data_ptr(), csr.col.data_ptr(), einfo.data_ptr()
                sw.h_src, sw.v_src, sw.edge_params = h_src.data_ptr(), v_src.data_ptr(), ep.data_ptr()
                sw.E, sw.n_src, sw.ldh_src, sw.ldv, sw.v_off = csr.E, h_src.size(0), h_src.stride(0), v_src.stride(0), v_off
                sw.v_block_major = int(v_bm)
            a.x_dst, a.h_dst, a.c_in = x_dst.data_ptr(), h_dst.data_ptr(), c_in.data_ptr()
            a.h_out, a.c_out = h_out.data_ptr(), c_out.data_ptr()
            a.wstream, a.w2_tail = wstream.data_ptr(), w2_tail.data_ptr()
            # (optional last element of a problem: the caller's own flag word -- a rollout's -- instead of the device-wide one)
            a.flags = (rest[0] if rest and rest[0] is not None else self.range_flag(x_dst.device)).data_ptr()
            a.n_dst, a.ldx, a.ldh, a.n_in, a.f_dst = n, x_dst.stride(0), h_dst.stride(0), n_in, x_dst.size(1)
        self._launch(self.lib.ggnn_decoder_cell_batch, "ggnn_decoder_cell_batch", arr, len(problems),
                     _lib.current_stream())

    def aggregate_backward(self, csr, rcsr, r_slot, einfo, p_src, p_dst, h_src, ep, agg, g_agg,
                           v_off, u_off, u4_off, a_off, a_gstride, sc_off, n_gates, out_p_dst=None, out_p_src=None,
                           ep_partial_out=None, g_h_into=None, inputs=None):
        """ggnn_period_gat_aggregate_backward (include/ggnn.h).  `rcsr`: CSR of the flipped
        edge_index (grouped by source), `r_slot` [E] int32: forward CSR slot of every reverse slot.
        Returns (g_p_dst, g_p_src, g_h_src or None, g_ep [n_gates, 3, 96]); the gradient tensors
        have the layout of their operands, columns the sweep does not read are zero.
        `ep_partial_out` [>= aggregate_bwd_partials(n_dst), n_gates, 3, 96]: the per-workgroup partial sums of g_ep go
        there and g_ep is returned as None -- the caller sums them (one reduction for the sweeps of a cell).
        `g_h_into` [n_src, 96]: an earlier sweep's g_h_src of the same source node type -- this sweep ADDS its own to it in
        place (g_h_accumulate) and returns it.
        `inputs` = (f_src, g_x_src [n_src, >= f_src], g_x_dst [n_dst, >= 3], g_edge_attr [edges of the list], src_accumulate,
        dst_accumulate): the input gradients of ggnn_period_gat_aggregate_backward_inputs go into these float32 buffers
        (columns 0..f_src-1 of the source rows, 0..2 of the destination rows, every kept edge's attribute; the flags add to
        what the rows hold).  None: the entry point and the kernels without them."""
        _require_cuda(csr.rowptr, rcsr.rowptr, r_slot, einfo, p_src, p_dst, h_src, ep, agg, g_agg)
        dev = p_src.device
        E, G = csr.E, n_gates
        a = AggregateBwdArgs()
        a.rowptr, a.col, a.einfo = csr.rowptr.data_ptr(), csr.col.data_ptr(), einfo.data_ptr()
        a.p_src, a.p_dst = p_src.data_ptr(), p_dst.data_ptr()
        a.h_src = None if h_src is None else h_src.data_ptr()
        a.edge_params, a.agg, a.g_agg = ep.data_ptr(), agg.data_ptr(), g_agg.data_ptr()
        a.r_rowptr, a.r_dst, a.r_slot = rcsr.rowptr.data_ptr(), rcsr.col.data_ptr(), r_slot.data_ptr()
        if agg.stride(0) != g_agg.stride(0) or agg.shape != g_agg.shape:
            raise _lib.GGNNError("g_agg must have the layout of agg")
        n_part = self.lib.ggnn_aggregate_bwd_partials(p_dst.size(0))
        f32 = dict(dtype=torch.float32, device=dev)
        scratch = torch.empty(2, max(E, 1) * G, **f32)
        if ep_partial_out is None:
            ep_partial = torch.empty(n_part, G, _lib.GGNN_EDGE_PARAM_ROWS, 96, **f32)
        else:
            ep_partial = ep_partial_out
            if not ep_partial.is_contiguous() or ep_partial.dtype != torch.float32 \
                    or tuple(ep_partial.shape[1:]) != (G, _lib.GGNN_EDGE_PARAM_ROWS, 96) or ep_partial.size(0) < n_part:
                raise _lib.GGNNError("ep_partial_out must be a contiguous [>= partials, n_gates, 3, 96] float32 tensor")
        # out_p_dst / out_p_src: zero-initialised gradient buffers shared by the sweeps of a cell (every
        # sweep writes its own columns only)
        g_p_dst = torch.zeros_like(p_dst) if out_p_dst is None else out_p_dst
        g_p_src = torch.zeros_like(p_src) if out_p_src is None else out_p_src
        if g_p_dst.shape != p_dst.shape or g_p_src.shape != p_src.shape or g_p_dst.stride(0) != p_dst.stride(0) \
                or g_p_src.stride(0) != p_src.stride(0):
            raise _lib.GGNNError("gradient buffers must have the layout of their operands")
        if g_h_into is not None and (h_src is None or g_h_into.shape != h_src.shape or not g_h_into.is_contiguous()
                                     or g_h_into.dtype != torch.float32):
            raise _lib.GGNNError("g_h_into must be a contiguous float32 tensor of h_src's shape")
        g_h_src = None if h_src is None else (g_h_into if g_h_into is not None else torch.empty(h_src.shape, **f32))
        a.g_h_accumulate = 1 if g_h_into is not None else 0
        a.edge_alpha, a.edge_ds, a.ep_partial = scratch[0].data_ptr(), scratch[1].data_ptr(), ep_partial.data_ptr()
        a.g_p_dst, a.g_p_src = g_p_dst.data_ptr(), g_p_src.data_ptr()
        a.g_h_src = None if g_h_src is None else g_h_src.data_ptr()
        a.ldp_src, a.ldp_dst, a.ld_agg = p_src.stride(0), p_dst.stride(0), agg.stride(0)
        a.ldh_src = 0 if h_src is None else h_src.stride(0)
        if g_h_src is not None and h_src.stride(0) != g_h_src.stride(0):
            raise _lib.GGNNError("aggregate_backward: h_src rows must be contiguous (g_h_src has its layout)")
        a.n_src, a.n_dst, a.E, a.n_partials = p_src.size(0), p_dst.size(0), E, n_part
        a.v_off, a.u_off, a.u4_off, a.a_off, a.a_gstride, a.sc_off, a.n_gates = (
            v_off, u_off, u4_off, a_off, a_gstride, sc_off, n_gates)
        if inputs is not None:
            f_src, g_x_src, g_x_dst, g_ea, acc_s, acc_d = inputs
            _require_cuda(g_x_src, g_x_dst, g_ea, csr.perm)
            for t, rows, cols, name in ((g_x_src, p_src.size(0), f_src, "g_x_src"), (g_x_dst, p_dst.size(0), 3, "g_x_dst")):
                if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.size(0) != rows or t.size(1) < cols:
                    raise _lib.GGNNError(f"aggregate_backward: {name} must be float32 [{rows}, >= {cols}] with unit column stride")
            if g_ea.dtype != torch.float32 or not g_ea.is_contiguous() or g_ea.numel() < E:
                raise _lib.GGNNError("aggregate_backward: g_edge_attr must be a contiguous float32 tensor over the list's edges")
            if E and int(csr.perm.numel()) < E:
                raise _lib.GGNNError("aggregate_backward: the CSR's perm does not cover its slots")
            x = _lib.AggregateBwdInputs()
            edge_grad = torch.empty(max(E, 1), 16, **f32)
            x.perm, x.edge_grad = csr.perm.data_ptr(), edge_grad.data_ptr()
            ea_out = g_ea if g_ea.numel() else torch.empty(1, **f32)   # (a list without edges: nothing is written)
            x.g_x_src, x.g_x_dst, x.g_edge_attr = g_x_src.data_ptr(), g_x_dst.data_ptr(), ea_out.data_ptr()
            x.ldgx_src, x.ldgx_dst, x.f_src = g_x_src.stride(0), g_x_dst.stride(0), f_src
            x.g_x_src_accumulate, x.g_x_dst_accumulate = int(bool(acc_s)), int(bool(acc_d))
            self._launch(self.lib.ggnn_period_gat_aggregate_backward_inputs, "ggnn_period_gat_aggregate_backward_inputs",
                         ctypes.byref(a), ctypes.byref(x), _lib.current_stream())
            return g_p_dst, g_p_src, g_h_src, (ep_partial.sum(0) if ep_partial_out is None else None)
        self._launch(self.lib.ggnn_period_gat_aggregate_backward, "ggnn_period_gat_aggregate_backward", ctypes.byref(a),
                     _lib.current_stream())
        return g_p_dst, g_p_src, g_h_src, (ep_partial.sum(0) if ep_partial_out is None else None)

    def aggregate_bwd_partials(self, n_dst):
        """Rows of the partial-sum output one backward call writes (ggnn_aggregate_bwd_partials)."""
        return self.lib.ggnn_aggregate_bwd_partials(n_dst)

    # -- gate GEMM + LSTM --------------------------------------------------------------
    @staticmethod
    def _epilogue_args(a, agg, w2, p_dst, s_off, c_in, h_out, c_out, raw_out, n_gates, mode,
                       w2_planes=None, g_stride=0):
        _require_cuda(agg, w2, p_dst, c_in, h_out, c_out, raw_out, w2_planes)
        a.agg, a.w2, a.p_dst = agg.data_ptr(), w2.data_ptr(), p_dst.data_ptr()
        a.c_in = None if c_in is None else c_in.data_ptr()
        a.h_out = None if h_out is None else h_out.data_ptr()
        a.c_out = None if c_out is None else c_out.data_ptr()
        a.raw_out = None if raw_out is None else raw_out.data_ptr()
        a.ldp, a.N = p_dst.stride(0), agg.size(0)
        a.Ka, a.s_off, a.n_gates, a.mode = w2.size(2), s_off, n_gates, mode
        if g_stride:  # agg gate stride (floats) when the rows are padded; 0 = packed [N, n_gates * Ka]
            a.g_stride, a.ld_agg = g_stride, agg.stride(0)
        if w2_planes is not None:
            if w2_planes.dtype != torch.int16 or w2_planes.numel() != 2 * w2.size(0) * _lib.GGNN_C * (w2.size(2) - 4):
                raise _lib.GGNNError("w2_planes does not match w2 (see packing.bf16_planes)")
            a.w2_planes = w2_planes.data_ptr()

    def lstm_epilogue(self, agg, w2, p_dst, s_off, c_in, h_out, c_out, raw_out, n_gates, mode, w2_planes=None, g_stride=0):
        """w2_planes: packing.bf16_planes(w2) (selects the bf16x6 kernel unless GGNN_GEMM=fp32)."""
        self.lstm_epilogue_batch([(agg, w2, p_dst, s_off, c_in, h_out, c_out, raw_out, n_gates, mode, w2_planes, g_stride)])

    def lstm_epilogue_batch(self, problems):
        """Up to four gate GEMM + LSTM problems (node types of a cell and / or both models) in one
        launch (ggnn_lstm_epilogue_batch); each item is the argument tuple of `lstm_epilogue`."""
        arr = (EpilogueArgs * len(problems))()
        for a, prob in zip(arr, problems):
            self._epilogue_args(a, *prob)
        self._launch(self.lib.ggnn_lstm_epilogue_batch, "ggnn_lstm_epilogue_batch", arr, len(problems),
                     _lib.current_stream())

    # -- LSTM update of the training path -----------------------------------------------
    def lstm_train_forward(self, z, p_dst, s_off, c_in, h_out, c_out):
        """One problem of lstm_train_forward_batch: z [G, N, 96] (gate GEMM output in, pre-activations out)."""
        self.lstm_train_forward_batch([(z, p_dst, s_off, c_in, h_out, c_out)], z.size(0))

    def lstm_train_backward(self, z, c_in, c_out, g_h, g_c, g_z, g_p_dst, s_off, g_c_in):
        """One problem of lstm_train_backward_batch (no padding columns): g_h / g_c / g_p_dst / g_c_in may be None."""
        self.lstm_train_backward_batch([(z, c_in, c_out, g_h, g_c, g_z, g_p_dst, s_off, g_c_in, 0, 0)], z.size(0))

    def lstm_train_forward_batch(self, problems, n_gates):
        """ggnn_lstm_train_forward_batch: [(z [G, N, 96], p_dst, s_off, c_in or None, h_out, c_out)] -- the node types of a
        cell in one launch."""
        arr = (_lib.LstmTrainProblem * len(problems))()
        for a, (z, p_dst, s_off, c_in, h_out, c_out) in zip(arr, problems):
            _require_cuda(z, p_dst, c_in, h_out, c_out)
            if not z.is_contiguous() or z.dim() != 3 or z.size(0) != n_gates or z.size(2) != _lib.GGNN_C \
                    or not (h_out.is_contiguous() and c_out.is_contiguous()) or (c_in is not None and not c_in.is_contiguous()):
                raise _lib.GGNNError("z [G, N, 96], c_in, h_out, c_out [N, 96] must be contiguous")
            a.z, a.p_dst, a.c_in, a.h_out, a.c_out = ptr(z), ptr(p_dst), ptr(c_in), ptr(h_out), ptr(c_out)
            a.ldp, a.N, a.s_off = p_dst.stride(0), z.size(1), s_off
        self._launch(self.lib.ggnn_lstm_train_forward_batch, "ggnn_lstm_train_forward_batch", arr, len(problems), n_gates,
                     _lib.current_stream())

    def lstm_train_backward_batch(self, problems, n_gates):
        """ggnn_lstm_train_backward_batch: [(z, c_in, c_out, g_h, g_c, g_z, g_p_dst, s_off, g_c_in, pad_off, pad_n)]; the
        call also zeroes g_p_dst[:, pad_off : pad_off + pad_n] (pad_n <= 96, multiples of 4)."""
        arr = (_lib.LstmTrainProblem * len(problems))()
        for a, (z, c_in, c_out, g_h, g_c, g_z, g_p_dst, s_off, g_c_in, pad_off, pad_n) in zip(arr, problems):
            _require_cuda(z, c_in, c_out, g_h, g_c, g_z, g_p_dst, g_c_in)
            for t in (z, c_in, c_out, g_h, g_c, g_z, g_c_in):
                if t is not None and not t.is_contiguous():
                    raise _lib.GGNNError("lstm_train_backward: z, g_z [G, N, 96] and the [N, 96] operands must be contiguous")
            if g_z.shape != z.shape or z.dim() != 3 or z.size(0) != n_gates:
                raise _lib.GGNNError("g_z must have the shape of z [G, N, 96]")
            a.z, a.c_in, a.c_out, a.g_h, a.g_c = ptr(z), ptr(c_in), ptr(c_out), ptr(g_h), ptr(g_c)
            a.g_z, a.g_p_dst, a.g_c_in = ptr(g_z), ptr(g_p_dst), ptr(g_c_in)
            a.ldp, a.N, a.s_off = 0 if g_p_dst is None else g_p_dst.stride(0), z.size(1), s_off
            a.pad_off, a.pad_n = pad_off, pad_n
        self._launch(self.lib.ggnn_lstm_train_backward_batch, "ggnn_lstm_train_backward_batch", arr, len(problems), n_gates,
                     _lib.current_stream())

    def train_input_rows(self, problems):
        """ggnn_train_input_rows: [(x [N, >= F], F)] -> [out [N, roundup4(F) + 4] = [x[:, :F] | 0 .. | 1 0 0 0]] in one launch."""
        arr = (_lib.TrainRowsProblem * len(problems))()
        outs = []
        for a, (x, F) in zip(arr, problems):
            _require_cuda(x)
            if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or x.size(1) < F:
                raise _lib.GGNNError("ggnn_train_input_rows: x must be float32 [N, >= F] with unit column stride")
            out = torch.empty(x.size(0), ((F + 3) & ~3) + 4, dtype=torch.float32, device=x.device)
            outs.append(out)
            a.x, a.out, a.ldx, a.ldo, a.N, a.F = ptr(x), ptr(out), x.stride(0), out.stride(0), x.size(0), F
        self._launch(self.lib.ggnn_train_input_rows, "ggnn_train_input_rows", arr, len(problems), _lib.current_stream())
        return outs

    def wgrad(self, a, b, K, M, Nc, lda, ldb, batch=1, a_bstride=0, b_bstride=0, b_ins=None, ins_off=0, defer=None):
        """ggnn_wgrad: C[batch, M, Nc] = A_k^T B_k; A_k = K rows of M floats, row pitch lda, from element
        k * a_bstride of the contiguous tensor `a` on (B_k likewise).  Returns the sum over the splits.
        `b_ins` [K, w] (contiguous): B is `b` with these w columns inserted at column ins_off (Nc counts them).
        `defer` (a list): the sum over the splits is NOT made by this call -- the returned tensor is filled by
        `sum_rows_batch(defer)`, which the caller runs once for several postponed reductions."""
        _require_cuda(a, b, b_ins)
        ins_w = 0
        if b_ins is not None:
            if b_ins.dtype != torch.float32 or b_ins.dim() != 2 or not b_ins.is_contiguous() or b_ins.size(0) < K or batch != 1:
                raise _lib.GGNNError("wgrad: b_ins must be a contiguous float32 [K, w] matrix (batch 1)")
            ins_w = b_ins.size(1)
        for t, ld, bs, w in ((a, lda, a_bstride, M), (b, ldb, b_bstride, Nc - ins_w)):
            if t.dtype != torch.float32 or not t.is_contiguous() or ld < w \
                    or (batch - 1) * bs + (K - 1) * ld + w > t.numel():
                raise _lib.GGNNError("wgrad: operands must be contiguous float32 tensors that hold every addressed row")
        S = self.lib.ggnn_wgrad_splits(K, M, Nc, batch)
        partial = torch.empty(S, batch, M, Nc, dtype=torch.float32, device=a.device)
        out = torch.empty(batch, M, Nc, dtype=torch.float32, device=a.device) if S > 1 else None
        w = _lib.WgradArgs()
        w.a, w.b, w.partial, w.out = a.data_ptr(), b.data_ptr(), partial.data_ptr(), (None if defer is not None else ptr(out))
        if defer is not None and S > 1:
            defer.append((partial.view(1, S, -1), out.view(1, -1)))
        w.lda, w.ldb, w.a_bstride, w.b_bstride, w.K = lda, ldb, a_bstride, b_bstride, K
        w.M, w.Nc, w.batch, w.n_split = M, Nc, batch, S
        if b_ins is not None:
            w.b_ins, w.ld_ins, w.ins_off, w.ins_w = b_ins.data_ptr(), b_ins.stride(0), ins_off, ins_w
        self._launch(self.lib.ggnn_wgrad, "ggnn_wgrad", ctypes.byref(w), _lib.current_stream())
        return out if S > 1 else partial[0]

    @staticmethod
    def _rowgemm_weight(g, w, K, n_out, batch, transposed, bf16):
        if w.dim() == 2:
            w = w.unsqueeze(0)
        if w.dtype != torch.float32 or w.dim() != 3 or w.stride(2) != 1 or w.size(0) != batch:
            raise _lib.GGNNError("ggnn_rowgemm: w must be a float32 [batch, rows, cols] view with unit column stride")
        if (transposed and (w.size(1) < K or w.size(2) < n_out)) or (not transposed and (w.size(1) < n_out or w.size(2) < K)):
            raise _lib.GGNNError("ggnn_rowgemm: w does not hold [n_out, K] (or its transpose)")
        g.w, g.w_bstride = w.data_ptr(), (w.stride(0) if batch > 1 else 0)
        g.w_nstride, g.w_kstride = (1, w.stride(1)) if transposed else (w.stride(1), 1)
        g.K, g.n_out, g.batch, g.precision = K, n_out, batch, _lib.GGNN_PRECISION_BF16 if bf16 else 0

    def rowgemm_pack(self, weights):
        """ggnn_rowgemm_pack: the weight planes of several ggnn_rowgemm products in ONE launch.  `weights` = [(w, K, n_out,
        batch, transposed, bf16)] as `rowgemm` takes them; returns one plane tensor per product for `rowgemm(..., planes=)`
        (fresh tensors: they may be kept until the backward pass)."""
        out = []
        for i0 in range(0, len(weights), _lib.GGNN_ROWGEMM_MAX_PACK):
            chunk = weights[i0:i0 + _lib.GGNN_ROWGEMM_MAX_PACK]
            arr = (_lib.RowGemmArgs * len(chunk))()
            for g, (w, K, n_out, batch, transposed, bf16) in zip(arr, chunk):
                _require_cuda(w)
                self._rowgemm_weight(g, w, K, n_out, batch, transposed, bf16)
                nbytes = self.lib.ggnn_rowgemm_workspace_bytes(K, n_out, batch)
                ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=w.device)
                g.workspace, g.workspace_bytes = ws.data_ptr(), nbytes
                out.append(ws)
            self._launch(self.lib.ggnn_rowgemm_pack, "ggnn_rowgemm_pack", arr, len(chunk), _lib.current_stream())
        return out

    def _rowgemm_args(self, a, w, out, K, n_out, batch, c_in, transposed, bf16, planes):
        """The filled ggnn_rowgemm_args of one product (checks included) and the tensor holding its weight planes."""
        _require_cuda(a, w, out, c_in)
        if a.dim() == 2:
            a = a.unsqueeze(0)
        if out.dim() == 2:
            out = out.unsqueeze(0)
        if c_in is not None and c_in.dim() == 2:
            c_in = c_in.unsqueeze(0)
        for t, name in ((a, "a"), (out, "out"), (c_in, "c_in")):
            if t is not None and (t.dtype != torch.float32 or t.dim() != 3 or t.stride(2) != 1):
                raise _lib.GGNNError(f"ggnn_rowgemm: {name} must be a float32 [batch, rows, cols] view with unit column stride")
        M = a.size(1)
        if a.size(0) != batch or out.size(0) != batch or out.size(1) != M or a.size(2) < K \
                or out.size(2) < n_out or (c_in is not None and (c_in.shape != out.shape or c_in.stride() != out.stride())):
            raise _lib.GGNNError("ggnn_rowgemm: operand shapes do not match (batch, M, K, n_out)")
        g = _lib.RowGemmArgs()
        self._rowgemm_weight(g, w, K, n_out, batch, transposed, bf16)
        nbytes = self.lib.ggnn_rowgemm_workspace_bytes(K, n_out, batch)
        if planes is not None:
            if planes.dtype != torch.uint8 or planes.numel() < nbytes or planes.device != a.device:
                raise _lib.GGNNError("ggnn_rowgemm: `planes` is not the rowgemm_pack output of this product")
            ws, g.prepacked = planes, 1
        else:
            # one plane buffer per (device, stream, size): the calls on a stream are ordered
            key = (a.device, torch.cuda.current_stream(a.device).cuda_stream, nbytes)
            ws = self._rowgemm_ws.get(key)
            if ws is None:
                ws = self._rowgemm_ws[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=a.device)
        g.a, g.c = a.data_ptr(), out.data_ptr()
        g.c_in = None if c_in is None else c_in.data_ptr()
        g.workspace, g.workspace_bytes = ws.data_ptr(), nbytes
        g.M, g.lda, g.ldc = M, a.stride(1), out.stride(1)
        g.a_bstride, g.c_bstride = a.stride(0) if batch > 1 else 0, out.stride(0) if batch > 1 else 0
        return g, ws

    def rowgemm(self, a, w, out, K, n_out, batch=1, c_in=None, transposed=False, bf16=False, planes=None):
        """ggnn_rowgemm (include/ggnn.h): out[b] = a[b] . W[b]^T (+ c_in[b]) for b < batch.
        `a`   : [M, lda] (batch 1) or [batch, M, lda] float32 view with unit column stride: the first K columns;
        `w`   : [batch, n_out, >= K] (transposed=False: W[b] = w[b][:, :K]) or [batch, K, >= n_out] (transposed=True:
                W[b] = w[b][:, :n_out]^T -- a gradient uses the transpose of the forward's weight), or 2-D for batch 1;
        `out` : [M, ldc] / [batch, M, ldc] float32 view with unit column stride: its first n_out columns are written
                (returned as given: a [M, n] result must not come back as [1, M, n] -- autograd would sum_to_size it);
        `c_in`: optional, same layout as out (another tensor: a ragged last row tile is produced twice, after its first store);
        `planes`: the weight planes of exactly this (w, K, n_out, batch, transposed, bf16) from `rowgemm_pack`."""
        g, _ = self._rowgemm_args(a, w, out, K, n_out, batch, c_in, transposed, bf16, planes)
        self._launch(self.lib.ggnn_rowgemm, "ggnn_rowgemm", ctypes.byref(g), _lib.current_stream())
        return out

    def rowgemm_pair(self, first, second):
        """ggnn_rowgemm_pair: two LONG products side by side in one grid; each = (a, w, out, K, n_out, c_in, transposed, bf16,
        planes) with the planes from `rowgemm_pack` (batch 1).  Falls back to two calls where the C entry point would refuse
        (a product whose weight planes stay in LDS, different output widths or precisions)."""
        args = [self._rowgemm_args(a, w, out, K, n_out, 1, c_in, transposed, bf16, planes)[0]
                for (a, w, out, K, n_out, c_in, transposed, bf16, planes) in (first, second)]
        tiles = lambda n: 6 if n <= 96 else (8 if n <= 128 else 14)
        streams = lambda g: not (g.K // 32 <= (8 if g.n_out == 96 else 4) and g.n_out in (96, 128, 224)) \
            and not (g.precision == 0 and g.n_out > 128)
        if all(g.prepacked and streams(g) for g in args) and tiles(args[0].n_out) == tiles(args[1].n_out) \
                and args[0].precision == args[1].precision:
            arr = (_lib.RowGemmArgs * 2)(*args)
            self._launch(self.lib.ggnn_rowgemm_pair, "ggnn_rowgemm_pair", arr, _lib.current_stream())
        else:
            for g in args:
                self._launch(self.lib.ggnn_rowgemm, "ggnn_rowgemm", ctypes.byref(g), _lib.current_stream())
        return first[2], second[2]

    def sum_rows(self, t):
        """ggnn_sum_rows: [batch, rows, cols] contiguous float32 -> [batch, cols], the sum over the rows in a fixed order."""
        _require_cuda(t)
        if t.dtype != torch.float32 or t.dim() != 3 or not t.is_contiguous() or t.size(2) % 4:
            raise _lib.GGNNError("ggnn_sum_rows: a contiguous float32 [batch, rows, cols] tensor with cols % 4 == 0")
        out = torch.empty(t.size(0), t.size(2), dtype=torch.float32, device=t.device)
        self._launch(self.lib.ggnn_sum_rows, "ggnn_sum_rows", t.data_ptr(), out.data_ptr(), t.size(1), t.size(2), t.size(0),
                     _lib.current_stream())
        return out

    def sum_rows_batch(self, problems):
        """ggnn_sum_rows_batch: [(in [batch, rows, cols], out [batch, cols])] contiguous float32 -- out = the sum over the rows,
        all problems in one launch (chunks of GGNN_SUM_ROWS_MAX)."""
        for i0 in range(0, len(problems), _lib.GGNN_SUM_ROWS_MAX):
            chunk = problems[i0:i0 + _lib.GGNN_SUM_ROWS_MAX]
            arr = (_lib.SumRowsProblem * len(chunk))()
            for a, (t, out) in zip(arr, chunk):
                _require_cuda(t, out)
                if t.dtype != torch.float32 or t.dim() != 3 or not t.is_contiguous() or t.size(2) % 4 or out.dtype != torch.float32 \
                        or not out.is_contiguous() or out.numel() != t.size(0) * t.size(2):
                    raise _lib.GGNNError("ggnn_sum_rows_batch: contiguous float32 [batch, rows, cols] (cols % 4 == 0) -> [batch, cols]")
                a.in_, a.out, a.n_rows, a.n_cols, a.batch = t.data_ptr(), out.data_ptr(), t.size(1), t.size(2), t.size(0)
            self._launch(self.lib.ggnn_sum_rows_batch, "ggnn_sum_rows_batch", arr, len(chunk), _lib.current_stream())

    def adam_step(self, args):
        """ggnn_adam_step (include/ggnn.h) on a filled `_lib.AdamArgs` (training.FusedAdam builds it)."""
        self._launch(self.lib.ggnn_adam_step, "ggnn_adam_step", ctypes.byref(args), _lib.current_stream())

    @staticmethod
    def _pack_args(plan, flat2, kq, packed=None, params=None):
        a = _lib.PackArgs()
        if params is None:
            a.flat2, a.kq, a.kq_idx, a.idx3 = flat2.data_ptr(), kq.data_ptr(), plan.kq_idx.data_ptr(), plan.idx3.data_ptr()
        else:   # the parameters read where they lie: encoded index tables + the DEVICE table of their addresses
            if params.dtype != torch.int64 or params.numel() != len(plan.sizes) or not params.is_cuda:
                raise _lib.GGNNError("ggnn_pack_weights_batch: params must be a device int64 table with one address per parameter tensor")
            a.flat2, a.kq, a.kq_idx, a.idx3 = flat2.data_ptr(), kq.data_ptr(), plan.kq_idx_enc.data_ptr(), plan.idx3_enc.data_ptr()
            a.params = params.data_ptr()
        a.packed = 0 if packed is None else packed.data_ptr()
        a.n_flat, a.zero, a.n_packed = plan.n_flat, plan.zero, plan.n_packed
        a.nb, a.r, a.c, a.L = plan.mr_shape[0], plan.mr_shape[1], plan.mr_shape[2], plan.idx3.size(1)
        a.coef = plan.k_coef
        return a

    def pack_weights(self, plan, flat2, kq, packed, params=None):
        """One cell of pack_weights_batch: `flat2` [plan.n_flat2] holds the parameters in its first n_flat entries -- or, with `params` (a
        device int64 table of the parameter tensors' addresses), they are read where they lie and that part of flat2 is not
        touched; fills the operands `kq` [plan.n_kq], the products and `packed` [plan.n_packed] (train_pack._PackWeights)."""
        self.pack_weights_batch([(plan, flat2, kq, packed, params)])

    def pack_weights_batch(self, cells):
        """ggnn_pack_weights_batch: [(plan, flat2, kq, packed, params)] -- the cells of a step with every launch shared."""
        arr = (_lib.PackArgs * len(cells))()
        for k, (plan, flat2, kq, packed, params) in enumerate(cells):
            _require_cuda(flat2, kq, packed)
            if flat2.dtype != torch.float32 or packed.dtype != torch.float32 or kq.dtype != torch.float32 \
                    or flat2.numel() != plan.n_flat2 or kq.numel() != plan.n_kq or packed.numel() != plan.n_packed \
                    or not flat2.is_contiguous() or not packed.is_contiguous() or not kq.is_contiguous():
                raise _lib.GGNNError("ggnn_pack_weights_batch: flat2 [n_flat2], kq [n_kq] and packed [n_packed] must be contiguous float32")
            arr[k] = self._pack_args(plan, flat2, kq, packed, params)
        self._launch(self.lib.ggnn_pack_weights_batch, "ggnn_pack_weights_batch", arr, len(cells), _lib.current_stream())

    def pack_weights_backward(self, plan, flat2, kq, grads, g_flat2, g_kq, g_flat):
        """One cell of pack_weights_backward_batch: `grads` = the gradients of the nine packed outputs (None: zero), contiguous float32 of
        plan.out_sizes; workspaces g_flat2 [n_flat2], g_kq [n_kq]; g_flat [>= n_flat] receives the parameters' gradient in its
        first n_flat entries and zeros behind them (n_tail: the parameters without effect)."""
        self.pack_weights_backward_batch([(plan, flat2, kq, grads, g_flat2, g_kq, g_flat)])

    def pack_weights_backward_batch(self, cells):
        """ggnn_pack_weights_backward_batch: [(plan, flat2, kq, grads, g_flat2, g_kq, g_flat)], every launch shared."""
        arr = (_lib.PackBwdArgs * len(cells))()
        for k, (plan, flat2, kq, grads, g_flat2, g_kq, g_flat) in enumerate(cells):
            self._pack_bwd_args(arr[k], plan, flat2, kq, grads, g_flat2, g_kq, g_flat)
        self._launch(self.lib.ggnn_pack_weights_backward_batch, "ggnn_pack_weights_backward_batch", arr, len(cells),
                     _lib.current_stream())

    def _pack_bwd_args(self, b, plan, flat2, kq, grads, g_flat2, g_kq, g_flat):
        _require_cuda(flat2, g_flat2, g_kq, g_flat, *[g for g in grads if g is not None])
        if len(grads) != _lib.GGNN_PACK_OUTPUTS or g_flat2.numel() != plan.n_flat2 or g_kq.numel() != plan.n_kq \
                or g_flat.numel() < plan.n_flat or not g_flat.is_contiguous():
            raise _lib.GGNNError("ggnn_pack_weights_backward_batch: nine output gradients and workspaces of the plan's sizes")
        b.fwd = self._pack_args(plan, flat2, kq)
        b.fwd.packed = g_flat.data_ptr()   # (unused by the backward; must not be NULL)
        off = 0
        for s, (g, n) in enumerate(zip(grads, plan.out_sizes)):
            if g is not None and (g.dtype != torch.float32 or g.numel() != n):
                raise _lib.GGNNError("ggnn_pack_weights_backward_batch: output gradients must be float32 of the outputs' sizes")
            b.g_out[s] = None if g is None else g.data_ptr()
            b.g_off[s] = off
            off += n
            if g is None or g.is_contiguous():
                b.g_w[s], b.g_rs[s], b.g_cs[s] = max(n, 1), 0, 1
            elif g.dim() == 2:          # a column block of a wider matrix (or of its transpose): read in place
                b.g_w[s], b.g_rs[s], b.g_cs[s] = g.size(1), g.stride(0), g.stride(1)
            elif g.dim() == 1:          # a column of a matrix
                b.g_w[s], b.g_rs[s], b.g_cs[s] = 1, g.stride(0), 1
            else:
                raise _lib.GGNNError("ggnn_pack_weights_backward_batch: a non-contiguous output gradient must be 1-D or 2-D")
        b.g_off[_lib.GGNN_PACK_OUTPUTS] = off
        b.inv, b.inv_kq = plan.inv.data_ptr(), plan.inv_kq.data_ptr()
        b.g_flat2, b.g_kq, b.g_flat = g_flat2.data_ptr(), g_kq.data_ptr(), g_flat.data_ptr()
        b.n_flat2, b.n_kq, b.inv_m, b.inv_kq_m = plan.n_flat2, plan.n_kq, plan.inv.size(1), plan.inv_kq.size(1)
        b.n_tail = g_flat.numel() - plan.n_flat

    def masked_mse(self, terms, scale, loss, want_grad=True, rows=None):
        """ggnn_masked_mse: `terms` = [(pred, target, mask or None)], contiguous float32 CUDA tensors; mask has the shape
        of pred or one entry per leading row of it.  Returns the gradients [g_pred] (None each with want_grad=False).
        `rows`: per term None or an int64 [1] device tensor -- the number of real leading rows of a term whose tensors carry
        pad rows behind them (mask 0 there): the term's mean is taken over them (ggnn_masked_mse_rows)."""
        a = _lib.MseArgs()
        q = None
        if rows is not None and any(r is not None for r in rows):
            if len(rows) != len(terms):
                raise _lib.GGNNError("ggnn_masked_mse_rows: one row count (or None) per term")
            q = _lib.MseCounts()
            for k, ((p, _, _), r) in enumerate(zip(terms, rows)):
                if r is None:
                    continue
                _require_cuda(r)
                if r.dtype != torch.int64 or r.numel() != 1 or p.dim() < 1 or p.size(0) < 1:
                    raise _lib.GGNNError("ggnn_masked_mse_rows: a row count is an int64 [1] device tensor")
                q.rows[k], q.row_elems[k] = r.data_ptr(), p.numel() // p.size(0)
        if not 1 <= len(terms) <= _lib.GGNN_MSE_MAX_TERMS:
            raise _lib.GGNNError("ggnn_masked_mse: 1..%d terms" % _lib.GGNN_MSE_MAX_TERMS)
        grads = []
        for k, (p, y, m) in enumerate(terms):
            _require_cuda(p, y, m)
            for t in (p, y, m):
                if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
                    raise _lib.GGNNError("ggnn_masked_mse: operands must be contiguous float32 tensors")
            if y.shape != p.shape:
                raise _lib.GGNNError("ggnn_masked_mse: pred and target differ in shape")
            div = 1
            if m is not None and m.numel() != p.numel():
                if p.dim() < 1 or m.numel() != p.size(0) or p.numel() % max(m.numel(), 1):
                    raise _lib.GGNNError("ggnn_masked_mse: mask must match pred or its leading dimension")
                div = p.numel() // m.numel()
            g = torch.empty_like(p) if want_grad else None
            grads.append(g)
            a.pred[k], a.target[k], a.mask[k], a.g_pred[k] = p.data_ptr(), y.data_ptr(), ptr(m), ptr(g)
            a.n[k], a.mask_div[k] = p.numel(), div
        # one workspace per (device, stream): two losses in flight on different streams (a capture on a side stream beside
        # eager work, two models training in threads) must not share the arrival counter and the partial sums
        key = (loss.device, torch.cuda.current_stream(loss.device).cuda_stream)
        ws = self._mse_ws.get(key)
        if ws is None:
            ws = self._mse_ws[key] = torch.zeros(_lib.GGNN_MSE_BLOCKS + 1, dtype=torch.float64, device=loss.device)
        a.workspace, a.loss, a.scale, a.n_terms = ws.data_ptr(), loss.data_ptr(), scale, len(terms)
        if q is None:
            self._launch(self.lib.ggnn_masked_mse, "ggnn_masked_mse", ctypes.byref(a), _lib.current_stream())
        else:
            self._launch(self.lib.ggnn_masked_mse_rows, "ggnn_masked_mse_rows", ctypes.byref(a), ctypes.byref(q),
                         _lib.current_stream())
        return grads

    # -- device-resident mini-batches (batches.py) ---------------------------------------
    def collate_batch(self, args):
        """ggnn_collate_batch on a filled `_lib.CollateArgs` (batches.DeviceBatches keeps one: every address in it is fixed)."""
        self._launch(self.lib.ggnn_collate_batch, "ggnn_collate_batch", ctypes.byref(args), _lib.current_stream())

    def reverse_slots(self, items):
        """ggnn_reverse_slots: items = [(csr, rcsr, r_slot_out [E] int32, scratch [E] int32)], the forward and the reverse
        table of a list and the kept-slot word they share (csr.E_dev, None = all E slots)."""
        arr = (_lib.ReverseSlotsArgs * len(items))()
        for a, (csr, rcsr, r_slot, scratch) in zip(arr, items):
            _require_cuda(csr.perm, rcsr.perm, r_slot, scratch, csr.E_dev)
            E = csr.E
            for t in (r_slot, scratch):
                if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() < E:
                    raise _lib.GGNNError("ggnn_reverse_slots: r_slot and scratch are contiguous int32 [E] tensors")
            if rcsr.E != E or csr.perm.numel() < E or rcsr.perm.numel() < E:
                raise _lib.GGNNError("ggnn_reverse_slots: the two tables must be built from one list")
            a.perm, a.r_perm, a.r_slot, a.scratch = csr.perm.data_ptr(), rcsr.perm.data_ptr(), r_slot.data_ptr(), scratch.data_ptr()
            a.E_kept, a.E = ptr(csr.E_dev), E
        self._launch(self.lib.ggnn_reverse_slots, "ggnn_reverse_slots", arr, len(items), _lib.current_stream())

    def metric_record(self, acc, terms, with_norm, mode, score, label, label_mask, thresholds, loss=None):
        """ggnn_metric_record: one validation batch into the accumulator `acc` (int64 [F64_SLOTS + I64_SLOTS] on the
        device, graingraphnn_amd.metrics), one launch.  `terms` = [(pred, target, mask, col)]: float32 [n, c] with unit
        column stride, mask one float32 per row ([n] or [n, 1]); `score` float32 [n], `label` int64 [n], `label_mask`
        float32 per element (regressor mode) or None; `loss` a float32 device scalar or None."""
        a = _lib.MetricArgs()
        if len(terms) > _lib.GGNN_METRIC_MAX_TERMS or len(thresholds) > _lib.GGNN_METRIC_MAX_THR:
            raise _lib.GGNNError("ggnn_metric_record: at most %d terms and %d thresholds"
                                 % (_lib.GGNN_METRIC_MAX_TERMS, _lib.GGNN_METRIC_MAX_THR))
        _require_cuda(acc, score, label, label_mask, loss)
        if acc.dtype != torch.int64 or not acc.is_contiguous() \
                or acc.numel() != _lib.GGNN_METRIC_F64_SLOTS + _lib.GGNN_METRIC_I64_SLOTS:
            raise _lib.GGNNError("ggnn_metric_record: the accumulator is %d contiguous 8-byte words"
                                 % (_lib.GGNN_METRIC_F64_SLOTS + _lib.GGNN_METRIC_I64_SLOTS))

        def rows(m, n, what):   # one float32 per row: -> its row stride
            if m.dtype != torch.float32 or m.dim() not in (1, 2) or m.size(0) != n or (n > 1 and m.stride(0) < 1):
                raise _lib.GGNNError(f"ggnn_metric_record: {what} must hold one float32 per row")
            return max(m.stride(0), 1)
        for k, (p, y, m, col) in enumerate(terms):
            _require_cuda(p, y, m)
            for t in (p, y):
                if t.dtype != torch.float32 or t.dim() != 2 or (t.numel() and t.size(1) > 1 and t.stride(1) != 1):
                    raise _lib.GGNNError("ggnn_metric_record: pred and target must be float32 [n, c] with unit column stride")
            n = p.size(0)
            if y.shape != p.shape or not 0 <= col < p.size(1) or (n > 1 and (p.stride(0) != y.stride(0) or p.stride(0) < p.size(1))):
                raise _lib.GGNNError("ggnn_metric_record: pred and target must agree in shape and row stride")
            a.pred[k], a.target[k], a.mask[k] = p.data_ptr(), y.data_ptr(), m.data_ptr()
            a.n_rows[k], a.ld[k], a.ld_mask[k], a.col[k] = n, max(p.stride(0), p.size(1)), rows(m, n, "mask"), col
        n = score.numel()
        if score.dtype != torch.float32 or not score.is_contiguous() or label.dtype != torch.int64 \
                or not label.is_contiguous() or label.numel() != n:
            raise _lib.GGNNError("ggnn_metric_record: score (float32) and label (int64) must be contiguous and of one length")
        a.score, a.label, a.n = score.data_ptr(), label.data_ptr(), n
        if label_mask is not None:
            a.label_mask, a.ld_label_mask = label_mask.data_ptr(), rows(label_mask, n, "label_mask")
        elif mode == _lib.METRIC_REGRESSOR:
            raise _lib.GGNNError("ggnn_metric_record: regressor mode needs the row mask")
        for j, t in enumerate(thresholds):
            a.thr[j] = t
        if loss is not None:
            if loss.dtype != torch.float32 or loss.numel() != 1:
                raise _lib.GGNNError("ggnn_metric_record: loss must be a float32 scalar on the device")
            a.loss = loss.data_ptr()
        # one workspace per (device, stream), as for ggnn_masked_mse: the arrival counter and the partial rows
        key = (acc.device, torch.cuda.current_stream(acc.device).cuda_stream)
        ws = self._metric_ws.get(key)
        if ws is None:
            ws = self._metric_ws[key] = torch.zeros(_lib.GGNN_METRIC_WS_WORDS, dtype=torch.int64, device=acc.device)
        a.acc, a.workspace = acc.data_ptr(), ws.data_ptr()
        a.n_terms, a.n_thr, a.mode, a.with_norm = len(terms), len(thresholds), mode, int(bool(with_norm))
        self._launch(self.lib.ggnn_metric_record, "ggnn_metric_record", ctypes.byref(a), _lib.current_stream())

    # -- heads -------------------------------------------------------------------------
    def heads_regressor(self, h_joint, h_grain, x_grain, w, b, y_joint, y_grain, grain_area):
        _require_cuda(h_joint, h_grain, x_grain, w, b, y_joint, y_grain, grain_area)
        check(self.lib.ggnn_heads_regressor(ptr(h_joint), h_joint.size(0), ptr(h_grain),
                                            h_grain.size(0), ptr(x_grain), x_grain.stride(0), ptr(w),
                                            ptr(b), ptr(y_joint), ptr(y_grain), ptr(grain_area),
                                            _lib.current_stream()), "ggnn_heads_regressor")

    def heads_regressor_backward(self, w, y_joint, y_grain, g_y_joint, g_y_grain, g_grain_area):
        """ggnn_heads_regressor_backward -> (g_pre_joint [n, 4], g_pre_grain [n, 4], g_h_joint, g_h_grain [n, 96]);
        the three incoming gradients may be None."""
        _require_cuda(w, y_joint, y_grain, g_y_joint, g_y_grain, g_grain_area)
        for t in (w, y_joint, y_grain, g_y_joint, g_y_grain, g_grain_area):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
                raise _lib.GGNNError("heads_regressor_backward: contiguous float32 operands")
        nj, ng = y_joint.size(0), y_grain.size(0)
        f32 = dict(dtype=torch.float32, device=w.device)
        gpj, gpg = torch.empty(nj, 4, **f32), torch.empty(ng, 4, **f32)
        ghj, ghg = torch.empty(nj, 96, **f32), torch.empty(ng, 96, **f32)
        self._launch(self.lib.ggnn_heads_regressor_backward, "ggnn_heads_regressor_backward", nj, ng, ptr(w), ptr(y_joint),
                     ptr(y_grain), ptr(g_y_joint), ptr(g_y_grain), ptr(g_grain_area), ptr(gpj), ptr(gpg), ptr(ghj),
                     ptr(ghg), _lib.current_stream())
        return gpj, gpg, ghj, ghg

    def heads_regressor_update(self, h_joint, h_grain, x_joint, x_grain, w, b, y_joint, y_grain, grain_area, dz, zmax,
                               flags):
        """heads_regressor + step_update in one launch (ggnn_heads_regressor_update)."""
        _require_cuda(h_joint, h_grain, x_joint, x_grain, w, b, y_joint, y_grain, grain_area, flags)
        self._launch(self.lib.ggnn_heads_regressor_update, "ggnn_heads_regressor_update", ptr(h_joint), h_joint.size(0),
                     ptr(h_grain), h_grain.size(0), ptr(x_joint), x_joint.stride(0), ptr(x_grain), x_grain.stride(0),
                     x_grain.size(1), ptr(w), ptr(b), ptr(y_joint), ptr(y_grain), ptr(grain_area), dz, zmax,
                     ptr(flags), _lib.current_stream())

    def step_refresh_prepare(self, x_joint, x_grain, zmax, flags, items, mirror=None):
        """step_refresh + edge_prepare of the next forward in one launch (ggnn_step_refresh_prepare); items as
        edge_prepare: (csr, edge_attr [E] COO order -- WRITTEN here --, x_src, x_dst, einfo_out).  `mirror` = (x_joint',
        x_grain'): second copies of the node features as they stand behind this call (include/ggnn.h)."""
        _require_cuda(x_joint, x_grain, flags)
        mj = mg = None
        if mirror is not None:
            mj, mg = mirror
            _require_cuda(mj, mg)
            if mj.shape != x_joint.shape or mg.shape != x_grain.shape or mj.stride() != x_joint.stride() \
                    or mg.stride() != x_grain.stride() or mj.dtype != torch.float32 or mg.dtype != torch.float32:
                raise _lib.GGNNError("mirror tensors must have the shape and strides of x_joint / x_grain")
        arr = _prepare_edges(items)
        self._launch(self.lib.ggnn_step_refresh_prepare, "ggnn_step_refresh_prepare", ptr(x_joint), x_joint.size(0),
                     x_joint.stride(0), ptr(x_grain), x_grain.size(0), x_grain.stride(0), zmax, ptr(flags), arr,
                     len(items), None if mj is None else ptr(mj), None if mg is None else ptr(mg), _lib.current_stream())

    def heads_classifier(self, h_joint, edge_index_jj, edge_attr_jj, w_node, w_edge, node_tmp,
                         edge_event, edge, E_dev=None):
        """`E_dev` (int64 [1], device): the number of edges at RUN time (edge_index_jj's own width is then the capacity the
        launch is sized for)."""
        _require_cuda(h_joint, edge_index_jj, edge_attr_jj, w_node, w_edge, node_tmp, edge_event, edge, E_dev)
        E = edge_index_jj.size(1)
        check(self.lib.ggnn_heads_classifier(ptr(h_joint), h_joint.size(0), ptr(edge_index_jj), E, ptr(E_dev),
                                             ptr(edge_attr_jj), ptr(w_node), ptr(w_edge),
                                             ptr(node_tmp), ptr(edge_event), ptr(edge),
                                             _lib.current_stream()), "ggnn_heads_classifier")

    # -- rollout-step glue -------------------------------------------------------------
    def step_update(self, x_joint, x_grain, y_joint, y_grain, dz, zmax, flags):
        _require_cuda(x_joint, x_grain, y_joint, y_grain, flags)
        check(self.lib.ggnn_step_update(ptr(x_joint), x_joint.size(0), x_joint.stride(0),
                                        ptr(x_grain), x_grain.size(0), x_grain.stride(0),
                                        x_grain.size(1), ptr(y_joint), ptr(y_grain), dz, zmax,
                                        ptr(flags), _lib.current_stream()), "ggnn_step_update")

    def grain_centres(self, csr_jg, x_joint, x_grain, domain_factor=1.0, domain_offset=None, centres_before=None,
                      boundary="periodic"):
        """x_grain[:, :2] <- region centres of the grains' junction polygons (graph.update(),
        graph_datastruct.py:681-708 + test.py:556-559).  csr_jg: CSR of (joint, pull, grain) (the FULL list for
        boundary="noflux": no min-image chaining, grain 0 included).  centres_before
        ([n_grain, 2] fp32, contiguous): receives x_grain[:, :2] as the call found them."""
        bc = _boundary_code(boundary)
        _require_cuda(x_joint, x_grain, csr_jg.rowptr, domain_offset, centres_before)
        if centres_before is not None:
            _f32c(centres_before, "centres_before")
            if tuple(centres_before.shape) != (x_grain.size(0), 2):
                raise _lib.GGNNError("centres_before must be [n_grain, 2]")
        if csr_jg.rowptr.numel() != x_grain.size(0) + 1:
            raise _lib.GGNNError("csr_jg must have one row per grain")
        if domain_offset is not None:
            _f32c(domain_offset, "domain_offset")
            if tuple(domain_offset.shape) != (x_joint.size(0), 2):
                raise _lib.GGNNError("domain_offset must be [n_joint, 2]")
        elif domain_factor > 1:
            raise _lib.GGNNError("domain_factor > 1 needs the domain_offset of scale_feature_patchs")
        check(self.lib.ggnn_grain_centres(ptr(csr_jg.rowptr), ptr(csr_jg.col), ptr(x_joint), x_joint.size(0),
                                          x_joint.stride(0), ptr(domain_offset), float(domain_factor), ptr(x_grain),
                                          x_grain.size(0), x_grain.stride(0), ptr(centres_before), bc,
                                          _lib.current_stream()), "ggnn_grain_centres")

    def noflux_boundary(self, csr_jg, x_joint, x_grain, domain_factor=1.0, domain_offset=None, max_y=1.0,
                        joints_before=None, traj_offsets=None):
        """The no-flux boundary step of test.py:446-463 (include/ggnn.h, ggnn_noflux_boundary): grain 0's features
        reset, its junctions (row 0 of csr_jg, the FULL joint->grain CSR) snapped to the nearest wall, every junction
        clamped to [0,1] x [0,max_y] in the global frame.  joints_before ([n_joint, 2] fp32): receives x_joint[:, :2]
        as the call found them.  traj_offsets: None, or (grain offsets, junction offsets), int64 [n_traj + 1] device
        tensors of a disjoint union whose caller has validated them (topology.check_noflux_union): every trajectory's
        first grain is its boundary grain (ggnn_noflux_boundary_traj)."""
        _require_cuda(x_joint, x_grain, csr_jg.rowptr, domain_offset, joints_before, *(traj_offsets or ()))
        _f32c(x_joint, "x_joint")
        _f32c(x_grain, "x_grain")
        if csr_jg.rowptr.numel() != x_grain.size(0) + 1:
            raise _lib.GGNNError("csr_jg must have one row per grain")
        for t, name in ((domain_offset, "domain_offset"), (joints_before, "joints_before")):
            if t is not None:
                _f32c(t, name)
                if tuple(t.shape) != (x_joint.size(0), 2):
                    raise _lib.GGNNError(f"{name} must be [n_joint, 2]")
        if domain_offset is None and domain_factor > 1:
            raise _lib.GGNNError("domain_factor > 1 needs the domain_offset of scale_feature_patchs")
        if traj_offsets is not None:
            og, oj = traj_offsets
            n_traj = _offsets((og, oj), "traj_offsets")
            check(self.lib.ggnn_noflux_boundary_traj(ptr(csr_jg.rowptr), ptr(csr_jg.col), ptr(x_joint), x_joint.size(0),
                                                     x_joint.stride(0), ptr(domain_offset), float(domain_factor),
                                                     float(max_y), ptr(x_grain), x_grain.stride(0), x_grain.size(1),
                                                     ptr(joints_before), ptr(og), ptr(oj), n_traj,
                                                     _lib.current_stream()), "ggnn_noflux_boundary_traj")
            return
        check(self.lib.ggnn_noflux_boundary(ptr(csr_jg.rowptr), ptr(csr_jg.col), ptr(x_joint), x_joint.size(0),
                                            x_joint.stride(0), ptr(domain_offset), float(domain_factor), float(max_y),
                                            ptr(x_grain), x_grain.stride(0), x_grain.size(1), ptr(joints_before),
                                            _lib.current_stream()), "ggnn_noflux_boundary")

    def qoi_accumulate(self, x_grain, live_grain, traj_offsets, const, state_in, state_out, V0, sync_word, flags,
                       history=None, capacity=0, area_sum=None, init=False, area0=None):
        """One layer of the rollout's quantities of interest (include/ggnn.h, ggnn_qoi_accumulate), one launch.
        const = (domain_factor, s, delta_h); state_in / state_out: dicts of fp32 [n_grain] `a`, `T`, `e` and the int32 word
        `layer` (the same dict twice: in place); V0 fp32 [n_grain] (written when `init`); history: None or fp32
        [capacity + 1, n_grain]; live_grain: int32 [n_grain] or None; traj_offsets: int64 [n_traj + 1] on the device."""
        n = x_grain.size(0)
        _require_cuda(x_grain, live_grain, traj_offsets, V0, sync_word, flags, history, area_sum, area0)
        _f32c(x_grain, "x_grain")
        for t, name in ((state_in["a"], "a_prev"), (state_in["T"], "T_in"), (state_out["a"], "a_cur"), (state_out["T"], "T_out"),
                        (state_out["e"], "e_cur"), (V0, "V0"), (area0, "area0")):
            if t is not None:
                _f32c(t, name)
                if t.numel() != n:
                    raise _lib.GGNNError(f"{name} must have one element per grain")
        n_traj = _offsets((traj_offsets,), "traj_offsets")
        if live_grain is not None and (live_grain.dtype != torch.int32 or live_grain.numel() != n):
            raise _lib.GGNNError("live_grain must be int32 [n_grain]")
        for w in (state_in["layer"], state_out["layer"], sync_word, flags):
            if w.dtype != torch.int32 or w.numel() < 1:
                raise _lib.GGNNError("layer / sync_word / flags must be int32 words")
        if history is not None:
            _f32c(history, "history")
            if history.numel() != (int(capacity) + 1) * n:
                raise _lib.GGNNError("history must be [capacity + 1, n_grain]")
        if area_sum is not None and (area_sum.dtype != torch.float32 or area_sum.numel() != n_traj):
            raise _lib.GGNNError("area_sum must be fp32 [n_traj]")
        A = _lib.QoiArgs()
        A.x_grain, A.live_grain, A.traj_offsets, A.area0 = ptr(x_grain), ptr(live_grain), ptr(traj_offsets), ptr(area0)
        A.a_prev, A.T_in, A.layer_in = ptr(state_in["a"]), ptr(state_in["T"]), ptr(state_in["layer"])
        A.a_cur, A.T_out, A.e_cur, A.layer_out = ptr(state_out["a"]), ptr(state_out["T"]), ptr(state_out["e"]), ptr(state_out["layer"])
        A.V0, A.history, A.area_sum, A.sync_word, A.flags = ptr(V0), ptr(history), ptr(area_sum), ptr(sync_word), ptr(flags)
        A.ldx_grain, A.n_grain, A.n_traj, A.capacity = x_grain.stride(0), n, n_traj, int(capacity)
        A.domain_factor, A.s, A.delta_h = (float(c) for c in const)
        A.init = 1 if init else 0
        check(self.lib.ggnn_qoi_accumulate(ctypes.byref(A), _lib.current_stream()), "ggnn_qoi_accumulate")

    def polygon_arena(self, n_grain, n_edges, capacity, device):
        """The per-layer arrays ggnn_grain_polygons writes: `rowptr` int32 [capacity + 1, n_grain + 1], `joint_sorted` int32
        [capacity + 1, E], `xy_sorted` fp32 [capacity + 1, E, 2], `centre` fp32 [capacity + 1, n_grain, 2], `area` fp32
        [capacity + 1, n_grain].  Zeroed: what a shrunken table leaves unwritten behind its last entry reads as 0."""
        L, i32, f32 = int(capacity) + 1, dict(dtype=torch.int32, device=device), dict(dtype=torch.float32, device=device)
        return {"rowptr": torch.zeros(L, n_grain + 1, **i32), "joint_sorted": torch.zeros(L, n_edges, **i32),
                "xy_sorted": torch.zeros(L, n_edges, 2, **f32), "centre": torch.zeros(L, n_grain, 2, **f32),
                "area": torch.zeros(L, n_grain, **f32)}

    def grain_polygons(self, csr_jg, x_joint, arena=None, domain_factor=1.0, domain_offset=None, boundary="periodic",
                       traj_grain_off=None, layer_in=None, layer_out=None, sync_word=None, flags=None):
        """One layer of the grains' junction polygons (include/ggnn.h, ggnn_grain_polygons), one launch; returns the arena.
        csr_jg: the table grain_centres reads (the FULL one for boundary="noflux"); arena: a polygon_arena (None: one of a
        single layer for this table, and the layer is written to its row 0); traj_grain_off: None or int64 [n_traj + 1] on
        the device (noflux: every trajectory's first grain is reversed); layer_in / layer_out / sync_word / flags: int32
        device words -- row *layer_in + 1 is written and left in *layer_out (layer_in None: row 0)."""
        bc = _boundary_code(boundary)
        n_grain = csr_jg.rowptr.numel() - 1
        if arena is None:
            arena = self.polygon_arena(n_grain, csr_jg.col.numel(), 0, x_joint.device)
        _require_cuda(x_joint, csr_jg.rowptr, csr_jg.col, domain_offset, traj_grain_off, layer_in, layer_out, sync_word, flags,
                      *arena.values())
        L, E_cap = arena["joint_sorted"].shape
        for name, dtype, shape in (("rowptr", torch.int32, (L, n_grain + 1)), ("joint_sorted", torch.int32, (L, E_cap)),
                                   ("xy_sorted", torch.float32, (L, E_cap, 2)), ("centre", torch.float32, (L, n_grain, 2)),
                                   ("area", torch.float32, (L, n_grain))):
            t = arena[name]
            if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise _lib.GGNNError(f"arena[{name!r}] must be a contiguous {dtype} tensor of shape {shape}")
        if L < 1 or n_grain < 1 or csr_jg.col.numel() < E_cap:
            raise _lib.GGNNError("the arena has more entries per layer than the joint->grain table")
        if csr_jg.rowptr.dtype != torch.int32 or csr_jg.col.dtype != torch.int32:
            raise _lib.GGNNError("csr_jg must hold int32 tables")
        if x_joint.dtype != torch.float32 or x_joint.dim() != 2 or x_joint.stride(1) != 1:
            raise _lib.GGNNError("x_joint must be float32 [n_joint, >= 2] with unit column stride")
        if domain_offset is not None:
            _f32c(domain_offset, "domain_offset")
            if tuple(domain_offset.shape) != (x_joint.size(0), 2):
                raise _lib.GGNNError("domain_offset must be [n_joint, 2]")
        elif domain_factor > 1:
            raise _lib.GGNNError("domain_factor > 1 needs the domain_offset of scale_feature_patchs")
        n_traj = 1 if traj_grain_off is None else _offsets((traj_grain_off,), "traj_grain_off")
        for w in (layer_in, layer_out, sync_word, flags):
            if w is not None and (w.dtype != torch.int32 or w.numel() < 1):
                raise _lib.GGNNError("layer_in / layer_out / sync_word / flags must be int32 words")
        if layer_out is not None and (sync_word is None or flags is None):
            raise _lib.GGNNError("layer_out needs sync_word and flags")
        A = _lib.PolygonArgs()
        A.rowptr, A.col, A.x_joint, A.domain_offset = ptr(csr_jg.rowptr), ptr(csr_jg.col), ptr(x_joint), ptr(domain_offset)
        A.traj_grain_off, A.rowptr_out, A.joint_sorted = ptr(traj_grain_off), ptr(arena["rowptr"]), ptr(arena["joint_sorted"])
        A.xy_sorted, A.centre, A.area = ptr(arena["xy_sorted"]), ptr(arena["centre"]), ptr(arena["area"])
        A.layer_in, A.layer_out, A.sync_word, A.flags = ptr(layer_in), ptr(layer_out), ptr(sync_word), ptr(flags)
        A.n_joint, A.ldx_joint, A.n_grain, A.E_cap = x_joint.size(0), x_joint.stride(0), n_grain, E_cap
        A.n_traj, A.capacity, A.domain_factor, A.boundary = n_traj, L - 1, float(domain_factor), bc
        check(self.lib.ggnn_grain_polygons(ctypes.byref(A), _lib.current_stream()), "ggnn_grain_polygons")
        return arena

    def polygon_inputs_arena(self, n_joint, n_edges, capacity, device):
        """The two per-layer arrays ggnn_polygon_inputs writes beside a polygon_arena: `col` int32 [capacity + 1, E] and
        `joint_xy` fp32 [capacity + 1, n_joint, 2].  Zeroed."""
        L = int(capacity) + 1
        return {"col": torch.zeros(L, n_edges, dtype=torch.int32, device=device),
                "joint_xy": torch.zeros(L, n_joint, 2, dtype=torch.float32, device=device)}

    def polygon_inputs(self, csr_jg, x_joint, inputs, domain_factor=1.0, domain_offset=None, layer_in=None):
        """What a layer's grain_polygons launch reads, kept for interp_polygons (include/ggnn.h, ggnn_polygon_inputs), one
        launch in front of that launch: row *layer_in + 1 (None: row 0) of `inputs` (a polygon_inputs_arena) receives the
        table's columns and the junctions in the global frame.  The word is not advanced."""
        col_out, xy = inputs["col"], inputs["joint_xy"]
        _require_cuda(x_joint, csr_jg.col, domain_offset, layer_in, col_out, xy)
        if col_out.dtype != torch.int32 or col_out.dim() != 2 or not col_out.is_contiguous():
            raise _lib.GGNNError("inputs['col'] must be a contiguous int32 [layers, E]")
        L, E_cap = col_out.shape
        n_joint = x_joint.size(0)
        if xy.dtype != torch.float32 or tuple(xy.shape) != (L, n_joint, 2) or not xy.is_contiguous():
            raise _lib.GGNNError(f"inputs['joint_xy'] must be a contiguous float32 tensor of shape ({L}, {n_joint}, 2)")
        if L < 1 or csr_jg.col.dtype != torch.int32 or csr_jg.col.numel() < E_cap:
            raise _lib.GGNNError("the inputs have more entries per layer than the joint->grain table")
        if x_joint.dtype != torch.float32 or x_joint.dim() != 2 or x_joint.stride(1) != 1:
            raise _lib.GGNNError("x_joint must be float32 [n_joint, >= 2] with unit column stride")
        if domain_offset is not None:
            _f32c(domain_offset, "domain_offset")
            if tuple(domain_offset.shape) != (n_joint, 2):
                raise _lib.GGNNError("domain_offset must be [n_joint, 2]")
        elif domain_factor > 1:
            raise _lib.GGNNError("domain_factor > 1 needs the domain_offset of scale_feature_patchs")
        if layer_in is not None and (layer_in.dtype != torch.int32 or layer_in.numel() < 1):
            raise _lib.GGNNError("layer_in must be an int32 word")
        A = _lib.PolygonInputsArgs()
        A.col, A.x_joint, A.domain_offset, A.col_out = ptr(csr_jg.col), ptr(x_joint), ptr(domain_offset), ptr(col_out)
        A.joint_xy, A.layer_in = ptr(xy), ptr(layer_in)
        A.n_joint, A.ldx_joint, A.E_cap, A.capacity, A.domain_factor = n_joint, x_joint.stride(0), E_cap, L - 1, float(domain_factor)
        check(self.lib.ggnn_polygon_inputs(ctypes.byref(A), _lib.current_stream()), "ggnn_polygon_inputs")
        return inputs

    def interp_polygons(self, arena, inputs, jobs, layers, boundary="periodic", max_y=1.0, traj_grain_off=None, out=None):
        """Polygon records of in-between layers (include/ggnn.h, ggnn_interp_polygons): jobs = [(layer L, coefficient c)],
        each blended from rows L - 1 and L of `inputs` (a polygon_inputs_arena) with the table of the nearer layer
        (`arena`'s rowptr, `inputs`' col).  layers: the number of layers recorded (1 <= L <= layers).  Returns a
        polygon_arena of len(jobs) rows (`out`: the one to fill), which rasterize_polygons reads as it reads the recorder's;
        two or three launches per GGNN_INTERP_MAX_JOBS jobs."""
        bc = _boundary_code(boundary)
        rowptr, col, xy = arena["rowptr"], inputs["col"], inputs["joint_xy"]
        _require_cuda(rowptr, col, xy, traj_grain_off)
        if rowptr.dtype != torch.int32 or rowptr.dim() != 2 or rowptr.size(1) < 2 or not rowptr.is_contiguous():
            raise _lib.GGNNError("arena['rowptr'] must be a contiguous int32 [layers, n_grain + 1]")
        L_cap, n_grain = rowptr.size(0), rowptr.size(1) - 1
        if col.dtype != torch.int32 or col.dim() != 2 or col.size(0) != L_cap or not col.is_contiguous():
            raise _lib.GGNNError(f"inputs['col'] must be a contiguous int32 [{L_cap}, E]")
        if xy.dtype != torch.float32 or xy.dim() != 3 or xy.size(0) != L_cap or xy.size(1) < 1 or xy.size(2) != 2 \
                or not xy.is_contiguous():
            raise _lib.GGNNError(f"inputs['joint_xy'] must be a contiguous float32 [{L_cap}, n_joint, 2]")
        E_cap, n_joint = col.size(1), xy.size(1)
        try:
            jobs = [(int(k), float(c)) for k, c in jobs]
        except (TypeError, ValueError):
            raise _lib.GGNNError("jobs must be (layer, coefficient) pairs") from None
        layers = int(layers)
        if not jobs:
            raise _lib.GGNNError("interp_polygons needs at least one job")
        if not 1 <= layers <= L_cap - 1:
            raise _lib.GGNNError(f"{layers} recorded layers: an in-between layer needs two of the arena's {L_cap}")
        for k, c in jobs:
            if not 1 <= k <= layers:
                raise _lib.GGNNError(f"a job's layer must lie in 1..{layers}, got {k}")
            if not 0.0 <= c <= 1.0:
                raise _lib.GGNNError(f"a job's coefficient must lie in [0, 1], got {c}")
        n_traj = 1 if traj_grain_off is None else _offsets((traj_grain_off,), "traj_grain_off")
        dev = rowptr.device
        if out is None:
            out = self.polygon_arena(n_grain, E_cap, len(jobs) - 1, dev)
        _require_cuda(*out.values())
        for name, dtype, shape in (("rowptr", torch.int32, (len(jobs), n_grain + 1)), ("joint_sorted", torch.int32, (len(jobs), E_cap)),
                                   ("xy_sorted", torch.float32, (len(jobs), E_cap, 2)), ("centre", torch.float32, (len(jobs), n_grain, 2)),
                                   ("area", torch.float32, (len(jobs), n_grain))):
            t = out[name]
            if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise _lib.GGNNError(f"out[{name!r}] must be a contiguous {dtype} tensor of shape {shape}")
        work = torch.empty(min(len(jobs), _lib.GGNN_INTERP_MAX_JOBS), n_joint, 2, dtype=torch.float32, device=dev)
        for first in range(0, len(jobs), _lib.GGNN_INTERP_MAX_JOBS):
            part = jobs[first:first + _lib.GGNN_INTERP_MAX_JOBS]
            host_layer = (ctypes.c_int32 * len(part))(*[k for k, _ in part])
            host_coeff = (ctypes.c_double * len(part))(*[c for _, c in part])
            A = _lib.InterpArgs()
            A.rowptr, A.col, A.joint_xy, A.traj_grain_off, A.work = ptr(rowptr), ptr(col), ptr(xy), ptr(traj_grain_off), ptr(work)
            A.job_layer, A.job_coeff = ctypes.cast(host_layer, ctypes.c_void_p), ctypes.cast(host_coeff, ctypes.c_void_p)
            A.rowptr_out, A.joint_sorted = ptr(out["rowptr"][first:]), ptr(out["joint_sorted"][first:])
            A.xy_sorted, A.centre, A.area = ptr(out["xy_sorted"][first:]), ptr(out["centre"][first:]), ptr(out["area"][first:])
            A.n_joint, A.n_grain, A.E_cap, A.capacity, A.layers = n_joint, n_grain, E_cap, L_cap - 1, layers
            A.n_traj, A.n_jobs, A.max_y, A.boundary = n_traj, len(part), float(max_y), bc
            check(self.lib.ggnn_interp_polygons(ctypes.byref(A), _lib.current_stream()), "ggnn_interp_polygons")
        return out

    def rasterize_polygons(self, arena, size, layers=None, boundary="periodic", grains=None, traj_grain_off=None,
                           corner_grains=None, out=None):
        """The grain-ID images of arena rows (include/ggnn.h, ggnn_polygons_rasterize): int32 [L, ny, nx] (periodic: [L, nx,
        nx]), pixel = the highest grain index + 1 among the polygons that hold it, 0 = uncovered; zeroed and filled by the
        call.  arena: a polygon_arena as grain_polygons left it; size = (nx, ny); layers: the rows to draw (host integers;
        None: all of them); grains = (g0, g1): that range alone, ids counted from g0; traj_grain_off: None or int64
        [n_traj + 1] on the device (noflux: every trajectory's first grain is skipped); corner_grains: four ids for the
        uncovered pixels of a no-flux image; out: the image to fill."""
        bc = _boundary_code(boundary)
        rowptr, xy = arena["rowptr"], arena["xy_sorted"]
        _require_cuda(rowptr, xy, traj_grain_off, out)
        if rowptr.dtype != torch.int32 or rowptr.dim() != 2 or rowptr.size(1) < 2 or not rowptr.is_contiguous():
            raise _lib.GGNNError("arena['rowptr'] must be a contiguous int32 [layers, n_grain + 1]")
        L_cap, n_grain = rowptr.size(0), rowptr.size(1) - 1
        if xy.dtype != torch.float32 or xy.dim() != 3 or xy.size(0) != L_cap or xy.size(2) != 2 or not xy.is_contiguous():
            raise _lib.GGNNError(f"arena['xy_sorted'] must be a contiguous float32 tensor of shape ({L_cap}, E, 2)")
        try:
            nx, ny = (int(v) for v in size)
        except (TypeError, ValueError):
            raise _lib.GGNNError("size must be (nx, ny)") from None
        if not (0 < nx < 1 << 15 and 0 < ny < 1 << 15):
            raise _lib.GGNNError(f"size must lie in 1 .. {(1 << 15) - 1} in both directions, got {(nx, ny)}")
        rows = list(range(L_cap)) if layers is None else [int(k) for k in layers]
        if not rows or any(not 0 <= k < L_cap for k in rows):
            raise _lib.GGNNError(f"layers must name rows 0..{L_cap - 1} of the arena, at least one")
        g0, g1 = (0, n_grain) if grains is None else (int(grains[0]), int(grains[1]))
        if not 0 <= g0 <= g1 <= n_grain:
            raise _lib.GGNNError(f"grains must be a range inside 0..{n_grain}")
        n_traj = 1 if traj_grain_off is None else _offsets((traj_grain_off,), "traj_grain_off")
        if corner_grains is not None:
            if bc != _lib.BC_NOFLUX:
                raise _lib.GGNNError("corner_grains belong to a no-flux image")
            corner_grains = [int(c) for c in corner_grains]
            if len(corner_grains) != 4 or any(not -2 ** 31 <= c < 2 ** 31 for c in corner_grains):
                raise _lib.GGNNError("corner_grains must be four int32 ids")
        shape = (len(rows), nx, nx) if bc == _lib.BC_PERIODIC else (len(rows), ny, nx)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=rowptr.device)
        elif out.dtype != torch.int32 or tuple(out.shape) != shape or not out.is_contiguous():
            raise _lib.GGNNError(f"out must be a contiguous int32 tensor of shape {shape}")
        A = _lib.RasterArgs()
        host_rows = (ctypes.c_int32 * len(rows))(*rows)
        A.rowptr, A.xy_sorted, A.traj_grain_off, A.image = ptr(rowptr), ptr(xy), ptr(traj_grain_off), ptr(out)
        A.layers = ctypes.cast(host_rows, ctypes.c_void_p)
        A.n_grain, A.E_cap, A.capacity, A.n_traj = n_grain, xy.size(1), L_cap - 1, n_traj
        A.grain_begin, A.grain_end, A.n_layers, A.nx, A.ny = g0, g1, len(rows), nx, ny
        if corner_grains is not None:
            A.corner_grains, A.with_corners = (ctypes.c_int32 * 4)(*corner_grains), 1
        A.boundary = bc
        check(self.lib.ggnn_polygons_rasterize(ctypes.byref(A), _lib.current_stream()), "ggnn_polygons_rasterize")
        return out

    def image_compare(self, image, truth=None, n_grain=None, differing=None, counts=None):
        """Differing pixels and per-id pixel counts of an int32 image (include/ggnn.h, ggnn_image_compare), one launch;
        returns (differing, counts): int64 device tensors [1] (None without `truth`) and [n_grain + 1] (None without
        `n_grain`), ADDED to the ones passed in (None: fresh zeroed ones).  truth: int32, the image's shape."""
        _require_cuda(image, truth, differing, counts)
        if image.dtype != torch.int32 or not image.is_contiguous() or image.numel() < 1:
            raise _lib.GGNNError("image must be a contiguous int32 tensor with pixels")
        if truth is not None and (truth.dtype != torch.int32 or truth.shape != image.shape or not truth.is_contiguous()):
            raise _lib.GGNNError("truth must be a contiguous int32 tensor of the image's shape")
        if truth is None and n_grain is None:
            raise _lib.GGNNError("image_compare needs truth, n_grain or both")
        if n_grain is not None and not 0 <= int(n_grain) < 2 ** 31 - 1:
            raise _lib.GGNNError("n_grain must not be negative")
        i64 = dict(dtype=torch.int64, device=image.device)
        if truth is None:
            differing = None
        elif differing is None:
            differing = torch.zeros(1, **i64)
        elif differing.dtype != torch.int64 or differing.numel() != 1:
            raise _lib.GGNNError("differing must be one int64 word")
        if n_grain is None:
            counts = None
        elif counts is None:
            counts = torch.zeros(int(n_grain) + 1, **i64)
        elif counts.dtype != torch.int64 or counts.numel() != int(n_grain) + 1 or not counts.is_contiguous():
            raise _lib.GGNNError("counts must be a contiguous int64 [n_grain + 1]")
        check(self.lib.ggnn_image_compare(ptr(image), ptr(truth), image.numel(), 0 if n_grain is None else int(n_grain),
                                          ptr(differing), ptr(counts), _lib.current_stream()), "ggnn_image_compare")
        return differing, counts

    def process_schedule(self, x_joint, table, traj_joint_off, step_in, step_out, sync_word):
        """The (G, R) features of the step to come from a device-side table (include/ggnn.h, ggnn_process_schedule), one
        launch: x_joint[:, 3:5] <- table[min(max(*step_in + 1, 0), n_rows - 1), trajectory of the junction], *step_out <-
        *step_in + 1.  table: fp32 [n_rows, n_traj, 2]; traj_joint_off: int64 [n_traj + 1] on the device, or None (one
        trajectory); step_in / step_out / sync_word: int32 device words (step_in and step_out may be the same)."""
        _require_cuda(x_joint, table, traj_joint_off, step_in, step_out, sync_word)
        _f32c(x_joint, "x_joint")
        _f32c(table, "table")
        if table.dim() != 3 or table.size(2) != 2 or table.size(0) < 1 or table.size(1) < 1:
            raise _lib.GGNNError("table must be fp32 [n_rows, n_traj, 2]")
        if traj_joint_off is None:
            if table.size(1) != 1:
                raise _lib.GGNNError("a table of several trajectories needs traj_joint_off")
        else:
            _offsets((traj_joint_off,), "traj_joint_off", table.size(1) + 1)
        for w in (step_in, step_out, sync_word):
            if w.dtype != torch.int32 or w.numel() < 1:
                raise _lib.GGNNError("step_in / step_out / sync_word must be int32 words")
        check(self.lib.ggnn_process_schedule(ptr(x_joint), x_joint.size(0), x_joint.stride(0), ptr(table), table.size(0),
                                             table.size(1), ptr(traj_joint_off), ptr(step_in), ptr(step_out), ptr(sync_word),
                                             _lib.current_stream()), "ggnn_process_schedule")

    def qoi_finalize(self, V0, T, e, traj_offsets, mesh_size, bin_edges=None):
        """(volume [n_grain], size [n_grain], d_mu [n_traj], d_std [n_traj], counts [n_traj, n_edges - 1] int32 or None) of
        ggnn_qoi_finalize; bin_edges: ascending fp32 [n_edges] on the device, or None."""
        _require_cuda(V0, T, e, traj_offsets, bin_edges)
        n, n_traj = V0.numel(), _offsets((traj_offsets,), "traj_offsets")
        for t, name in ((V0, "V0"), (T, "T"), (e, "e")):
            _f32c(t, name)
            if t.numel() != n:
                raise _lib.GGNNError(f"{name} must have one element per grain")
        dev = V0.device
        volume, size = torch.empty(n, device=dev), torch.empty(n, device=dev)
        d_mu, d_std = torch.empty(n_traj, device=dev), torch.empty(n_traj, device=dev)
        n_edges, hist = 0, None
        if bin_edges is not None:
            _f32c(bin_edges, "bin_edges")
            n_edges = bin_edges.numel()
            hist = torch.zeros(n_traj, max(n_edges - 1, 0), dtype=torch.int32, device=dev)
        check(self.lib.ggnn_qoi_finalize(ptr(V0), ptr(T), ptr(e), n, ptr(traj_offsets), n_traj, float(mesh_size), ptr(bin_edges),
                                         n_edges, ptr(volume), ptr(size), ptr(d_mu), ptr(d_std), ptr(hist),
                                         _lib.current_stream()), "ggnn_qoi_finalize")
        return volume, size, d_mu, d_std, hist

    def detect_events(self, grain_area, live_grain, area_threshold, edge_event, edge_index_jj,
                      logit_threshold, flags, range_word=None, E_dev=None, skip_grain=-1):
        """flags[0:2] (int32, device) <- (#grain events, #switch candidates); with `range_word` (int32 [1]) flags[2] <- the
        word, which is cleared; `E_dev` (int64 [1], device): the number of junction edges at RUN time; `skip_grain`: a
        grain never counted (the no-flux boundary grain, 0; -1 = none); see ggnn.h."""
        _require_cuda(grain_area, live_grain, edge_event, edge_index_jj, flags, range_word, E_dev)
        if live_grain.dtype != torch.int32 or flags.dtype != torch.int32 or flags.numel() < (2 if range_word is None else 3):
            raise _lib.GGNNError("live_grain / flags must be int32 (flags: two words, three with a range word)")
        if range_word is not None and (range_word.dtype != torch.int32 or range_word.numel() < 1):
            raise _lib.GGNNError("range_word must be an int32 word")
        check(self.lib.ggnn_detect_events(ptr(grain_area), ptr(live_grain), grain_area.numel(),
                                          float(area_threshold), ptr(edge_event), ptr(edge_index_jj),
                                          edge_index_jj.size(1), ptr(E_dev), float(logit_threshold), ptr(flags),
                                          ptr(range_word), int(skip_grain), _lib.current_stream()), "ggnn_detect_events")

    def detect_events_traj(self, grain_area, live_grain, area_threshold, edge_event, edge_index_jj, logit_threshold,
                           traj_grain_off, traj_joint_off, counts, flags, ended=None, range_word=None, E_dev=None,
                           skip_local_grain=-1):
        """detect_events for a disjoint union (ggnn_detect_events_traj, see ggnn.h): traj_grain_off / traj_joint_off int64
        [n_traj + 1] on the device; counts int32 [n_traj, 2] <- (grain, switch) candidates per trajectory; flags[0:2] <- their
        totals; ended: int32 [n_traj] or None, a non-zero word keeps a trajectory's candidates out of both."""
        _require_cuda(grain_area, live_grain, edge_event, edge_index_jj, traj_grain_off, traj_joint_off, counts, flags, ended,
                      range_word, E_dev)
        n_traj = _offsets((traj_grain_off, traj_joint_off), "traj_grain_off / traj_joint_off")
        if live_grain.dtype != torch.int32 or flags.dtype != torch.int32 or flags.numel() < (2 if range_word is None else 3):
            raise _lib.GGNNError("live_grain / flags must be int32 (flags: two words, three with a range word)")
        if counts.dtype != torch.int32 or counts.numel() != 2 * n_traj or not counts.is_contiguous():
            raise _lib.GGNNError("counts must be a contiguous int32 [n_traj, 2]")
        if ended is not None and (ended.dtype != torch.int32 or ended.numel() != n_traj or not ended.is_contiguous()):
            raise _lib.GGNNError("ended must be a contiguous int32 [n_traj]")
        if range_word is not None and (range_word.dtype != torch.int32 or range_word.numel() < 1):
            raise _lib.GGNNError("range_word must be an int32 word")
        check(self.lib.ggnn_detect_events_traj(ptr(grain_area), ptr(live_grain), grain_area.numel(), float(area_threshold),
                                               ptr(edge_event), ptr(edge_index_jj), edge_index_jj.size(1), ptr(E_dev),
                                               float(logit_threshold), ptr(traj_grain_off), ptr(traj_joint_off), n_traj,
                                               ptr(ended), int(skip_local_grain), ptr(counts), ptr(flags), ptr(range_word),
                                               _lib.current_stream()), "ggnn_detect_events_traj")

    def step_refresh(self, x_joint, x_grain, zmax, flags, edges):
        """edges: list of (edge_index [2,E] int64, x_src, x_dst, edge_attr_out [E][, E_dev int64 [1] or None])."""
        _require_cuda(x_joint, x_grain, flags)
        arr = (RefreshEdge * max(len(edges), 1))()
        for k, (ei, xs, xd, ea, *rest) in enumerate(edges):
            _require_cuda(ei, xs, xd, ea)
            arr[k].E_dev = ptr(rest[0]) if rest else None
            arr[k].edge_index, arr[k].x_src, arr[k].x_dst = ei.data_ptr(), xs.data_ptr(), xd.data_ptr()
            arr[k].edge_attr = ea.data_ptr()
            arr[k].ldx_src, arr[k].ldx_dst = xs.stride(0), xd.stride(0)
            arr[k].n_src, arr[k].n_dst, arr[k].E = xs.size(0), xd.size(0), ei.size(1)
        check(self.lib.ggnn_step_refresh(ptr(x_joint), x_joint.size(0), x_joint.stride(0),
                                         ptr(x_grain), x_grain.size(0), x_grain.stride(0), zmax,
                                         ptr(flags), arr, len(edges), _lib.current_stream()),
              "ggnn_step_refresh")


def _boundary_code(boundary):
    codes = {"periodic": _lib.BC_PERIODIC, "noflux": _lib.BC_NOFLUX}
    if boundary not in codes:
        raise _lib.GGNNError(f"boundary must be 'periodic' or 'noflux', got {boundary!r}")
    return codes[boundary]


_default = None


def default_backend():
    global _default
    if _default is None:
        _default = HipBackend()
    return _default
