"""Event-driven topology update of the grain graph, host side: the binding of
`ggnn_topology_update` (include/ggnn.h, csrc/topology.hip -- host code in the C-ABI library).

It restates `GrainNN_classifier.update` of the reference (models.py:612-842 with its helpers
`delete_grain_index` :861-893, `switching_edge_index` :896-1051, `point_in_triangle` :1055-1070,
`periodic_move` :1103-1106) for the periodic, nucleation-free configuration every shipped script
runs (test.py:88 `--nucleation_density 0`).  The work is integer / index work on a few edges per
event and inherently sequential (every event rewires the lists the next one reads), so it runs on
the host between device steps; the device side only sees new `edge_index` tensors, for which
`engine.graph_for` rebuilds the CSR.

The reference answers every lookup with a mask over a whole edge list (57-75 ms of host time per
eventful step at the 10k-grain graph, measured with that formulation: oracle/topology_scan.py, now
the test oracle); the library answers them from column indices and running counts in native code
(profiles/r5_event_step_breakdown.txt).

Bit-exactness contract (tests/golden/golden_cfg1_events.npz, produced by the unmodified
reference): identical `edge_index` COLUMN ORDER (edges are rewritten in place, new edges are
appended, dead columns are dropped at the end -- never re-sorted), identical masks, identical
fp32 junction coordinates.
"""
import ctypes
import os
from typing import Optional, Sequence

import numpy as np

from . import _lib

GJ, JG, JJ = ("grain", "push", "joint"), ("joint", "pull", "grain"), ("joint", "connect", "joint")


class TopologyError(RuntimeError):
    """The lists are not a valid grain graph (the reference asserts / raises KeyError here)."""


def _flags(ids: Optional[Sequence[int]], n: int) -> Optional[np.ndarray]:
    """Index list of an active window -> one byte per node (None = everything is active)."""
    if ids is None:
        return None
    f = np.zeros(n, dtype=np.uint8)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    f[ids[(ids >= 0) & (ids < n)]] = 1
    return f


def _library():
    """libggnn.so -- or, for the sanitizer run of the host code only (tests/test_topology.py under
    `make -C graingraphnn_amd/csrc host-asan`), the plain-C++ build of csrc/topology.hip named by GGNN_TOPOLOGY_LIB."""
    alt = os.environ.get("GGNN_TOPOLOGY_LIB")
    if not alt:
        return _lib.load()
    lib = _alt_libs.get(alt)
    if lib is None:
        lib = _alt_libs[alt] = ctypes.CDLL(alt)
        c_int, c_int64, c_void_p, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER
        lib.ggnn_topology_update.restype = c_int
        lib.ggnn_topology_update.argtypes = [P(_lib.TopologyArgs)]
        lib.ggnn_topology_open.restype = c_int
        lib.ggnn_topology_open.argtypes = [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                           P(c_void_p), ctypes.c_char_p]
        lib.ggnn_topology_apply.restype = c_int
        lib.ggnn_topology_apply.argtypes = [c_void_p, P(_lib.TopologyArgs)]
        lib.ggnn_topology_counts.restype = c_int
        lib.ggnn_topology_counts.argtypes = [c_void_p, P(c_int64), P(c_int64)]
        lib.ggnn_topology_export.restype = c_int
        lib.ggnn_topology_export.argtypes = [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64]
        lib.ggnn_topology_close.restype = None
        lib.ggnn_topology_close.argtypes = [c_void_p]
    return lib


_alt_libs = {}
_p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class TopologySession:
    """The lists of ONE trajectory kept inside the library between updates (ggnn_topology_open / _apply / _export,
    include/ggnn.h): the reference's loop calls `Cmodel.update` at every step (test.py:418-426); the session keeps the
    lookup tables and per-grain counts and patches them as the events rewrite columns, so an update costs what its events
    touch.  Same results, bit for bit, as chained `update_topology` calls (tests/test_topology.py).

    `apply` works IN PLACE on the caller's x_joint / y_joint / masks (a refused update leaves them and the session
    untouched -- the library journals its writes); `export` writes the current lists into caller-provided int64 arrays
    (e.g. pinned staging buffers of an upload)."""

    def __init__(self, ei_jj: np.ndarray, ei_jg: np.ndarray, n_joint: int, n_grain: int):
        self._lib = _library()
        pp = np.ascontiguousarray(ei_jj, dtype=np.int64)
        pq = np.ascontiguousarray(ei_jg, dtype=np.int64)
        if pp.ndim != 2 or pp.shape[0] != 2 or pq.ndim != 2 or pq.shape[0] != 2:
            raise ValueError("edge lists must be [2, E]")
        self.n_joint, self.n_grain = int(n_joint), int(n_grain)
        self._h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(192)
        rc = self._lib.ggnn_topology_open(_p(pp), pp.shape[1], pp.shape[1], _p(pq), pq.shape[1], pq.shape[1],
                                          self.n_joint, self.n_grain, ctypes.byref(self._h), err)
        if rc == _lib.GGNN_ETOPOLOGY:
            raise TopologyError(err.value.decode(errors="replace"))
        _lib.check(rc, "ggnn_topology_open")
        self.n_pp, self.n_pq = pp.shape[1], pq.shape[1]
        # output lists of a call: sized once (a call reports at most every edge / every grain + the dead-column marker)
        self._switching = np.empty((max(self.n_pp, 1), 2), dtype=np.int64)
        self._extra = np.empty(self.n_grain + 1, dtype=np.int64)
        self._args = _lib.TopologyArgs()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ggnn_topology_close(self._h)
            self._h = None

    __del__ = close

    def apply(self, x_joint: np.ndarray, y_joint: np.ndarray, y_grain_area: np.ndarray, edge_prob: np.ndarray,
              grain_event, mask_grain: np.ndarray, mask_joint: np.ndarray, threshold: float,
              active_grain: Optional[np.ndarray] = None, active_joint: Optional[np.ndarray] = None):
        """One update.  x_joint [N_j, >= 8] / y_joint [N_j, 2] fp32 C-contiguous and the int64 masks (any shape with N
        elements, contiguous) are rewritten in place; y_grain_area = a float32 view whose element g is the predicted area
        change of grain g (e.g. y_grain[:, 0]: strided views are taken as they are); edge_prob [n_pp] float32;
        active_* = one byte per node or None.  Returns (grain events incl. forced ones, switching list [S, 2])."""
        n_j, n_g = self.n_joint, self.n_grain
        for name, a, shape in (("x_joint", x_joint, None), ("y_joint", y_joint, (n_j, 2))):
            if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 2 or a.shape[0] != n_j \
                    or not a.flags.c_contiguous or (shape is not None and a.shape != shape):
                raise ValueError(f"{name} must be a C-contiguous float32 array [{n_j}, {'2' if shape else '>= 8'}]")
        if x_joint.shape[1] < 8:
            raise ValueError("x_joint needs the 8 junction features (columns 6, 7 = the displacement the events reset)")
        for name, a, n in (("mask_grain", mask_grain, n_g), ("mask_joint", mask_joint, n_j)):
            if not isinstance(a, np.ndarray) or a.dtype != np.int64 or a.size != n or not a.flags.c_contiguous:
                raise ValueError(f"{name} must be a contiguous int64 array of {n} elements")
        area = y_grain_area
        if not isinstance(area, np.ndarray) or area.dtype != np.float32 or area.ndim != 1 or area.shape[0] != n_g \
                or area.strides[0] % 4:
            raise ValueError("y_grain_area must be a float32 vector with one element per grain")
        prob = np.ascontiguousarray(np.asarray(edge_prob, dtype=np.float32).reshape(-1))
        if prob.shape[0] != self.n_pp:
            raise ValueError(f"edge_prob needs one entry per junction edge ({self.n_pp})")
        ge = np.ascontiguousarray(np.asarray(grain_event, dtype=np.int64).reshape(-1))
        A = self._args
        A.pp = A.pq = None
        A.x_joint, A.y_joint, A.y_grain_area, A.edge_prob = _p(x_joint), _p(y_joint), _p(area), _p(prob)
        A.grain_event, A.mask_grain, A.mask_joint = _p(ge), _p(mask_grain), _p(mask_joint)
        A.active_grain, A.active_joint = _p(active_grain), _p(active_joint)
        A.switching, A.events_extra = _p(self._switching), _p(self._extra)
        A.n_joint, A.n_grain, A.ldx, A.ldyg, A.n_grain_event = n_j, n_g, x_joint.shape[1], area.strides[0] // 4, ge.shape[0]
        A.switching_cap, A.extra_cap, A.threshold = self._switching.shape[0], self._extra.shape[0], float(threshold)
        rc = self._lib.ggnn_topology_apply(self._h, ctypes.byref(A))
        if rc == _lib.GGNN_ETOPOLOGY:
            raise TopologyError(A.error.decode(errors="replace"))
        _lib.check(rc, "ggnn_topology_apply")
        self.n_pp, self.n_pq = int(A.n_pp), int(A.n_pq)
        events = np.concatenate([ge, self._extra[:A.n_extra]]) if A.n_extra else ge
        return events, self._switching[:A.n_switching].copy()

    def export(self, pp: Optional[np.ndarray] = None, pq: Optional[np.ndarray] = None, qp: Optional[np.ndarray] = None,
               at: Sequence[int] = (0, 0)):
        """The current lists into int64 arrays [2, >= n] whose rows are contiguous (row stride = shape[1] elements); with
        no arguments: three fresh arrays (ei_jj [2, n_pp], ei_jg [2, n_pq], ei_gj [2, n_pq]).  `at` = (first column of pp's
        window, first column of pq's and qp's): the lists land in a column window of a wider array (a union's lists)."""
        fresh = pp is None and pq is None and qp is None
        if fresh:
            pp = np.empty((2, self.n_pp), np.int64)
            pq = np.empty((2, self.n_pq), np.int64)
            qp = np.empty((2, self.n_pq), np.int64)
        at_pp, at_pq = int(at[0]), int(at[1])
        for a, n, lo in ((pp, self.n_pp, at_pp), (pq, self.n_pq, at_pq), (qp, self.n_pq, at_pq)):
            if a is not None and (a.dtype != np.int64 or a.ndim != 2 or a.shape[0] != 2 or lo < 0 or a.shape[1] < lo + n
                                  or not a.flags.c_contiguous):
                raise ValueError("export targets must be C-contiguous int64 arrays [2, >= n]")
        ld = lambda a: 0 if a is None else a.shape[1]
        win = lambda a, lo: None if a is None else ctypes.c_void_p(a.ctypes.data + 8 * lo)
        _lib.check(self._lib.ggnn_topology_export(self._h, win(pp, at_pp), ld(pp), win(pq, at_pq), ld(pq), win(qp, at_pq),
                                                  ld(qp)), "ggnn_topology_export")
        return (pp, pq, qp) if fresh else None


def union_edge_segments(edge_index, offsets_src, offsets_dst, what="edge list"):
    """The columns of a disjoint union's edge list [2, E] per trajectory: [n_traj + 1] rising column offsets.  Raises
    GGNNError unless every edge lies inside ONE trajectory (source in offsets_src's range t, destination in offsets_dst's
    range t) and the segments stand in trajectory order -- what the per-trajectory event loop relies on."""
    ei = np.asarray(edge_index, dtype=np.int64)
    off_s, off_d = np.asarray(offsets_src, np.int64).reshape(-1), np.asarray(offsets_dst, np.int64).reshape(-1)
    n_traj = off_s.size - 1
    if ei.ndim != 2 or ei.shape[0] != 2:
        raise _lib.GGNNError(f"{what}: must be [2, E]")
    if ei.size and (ei.min() < 0 or ei[0].max() >= off_s[-1] or ei[1].max() >= off_d[-1]):
        raise _lib.GGNNError(f"{what}: a node index is outside the union")
    ts = np.searchsorted(off_s, ei[0], side="right") - 1
    td = np.searchsorted(off_d, ei[1], side="right") - 1
    bad = np.flatnonzero(ts != td)
    if bad.size:
        k = int(bad[0])
        raise _lib.GGNNError(f"{what}: edge {k} ({int(ei[0, k])} -> {int(ei[1, k])}) crosses from trajectory {int(ts[k])} "
                             f"to trajectory {int(td[k])}: not a disjoint union")
    if (np.diff(ts) < 0).any():
        k = int(np.flatnonzero(np.diff(ts) < 0)[0]) + 1
        raise _lib.GGNNError(f"{what}: the segments are not in trajectory order (edge {k} of trajectory {int(ts[k])} stands "
                             f"behind one of trajectory {int(ts[k - 1])})")
    return np.searchsorted(ts, np.arange(n_traj + 1), side="left").astype(np.int64)


def check_traj_offsets(traj_offsets, n_grain: int, n_joint: int):
    """{'grain': [...], 'joint': [...]} -> two int64 arrays [n_traj + 1] rising from 0 to the node counts, or GGNNError."""
    try:
        og = np.asarray(traj_offsets["grain"], dtype=np.int64).reshape(-1)
        oj = np.asarray(traj_offsets["joint"], dtype=np.int64).reshape(-1)
    except (KeyError, TypeError, IndexError):
        raise _lib.GGNNError("traj_offsets must be {'grain': [n_traj + 1], 'joint': [n_traj + 1]}") from None
    for off, n, nt in ((og, n_grain, "grain"), (oj, n_joint, "joint")):
        if off.size < 2 or off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
            raise _lib.GGNNError(f"traj_offsets['{nt}'] must rise from 0 to the number of {nt}s ({n})")
    if og.size != oj.size:
        raise _lib.GGNNError("traj_offsets: 'grain' and 'joint' must list the same number of trajectories")
    return og, oj


def check_noflux_union(grain_off, joint_off):
    """A no-flux union's offsets (check_traj_offsets' arrays): every trajectory's local grain 0 is its boundary grain, so a
    trajectory with junctions must own at least one grain (and one with grains has junctions: the boundary step reaches a
    trajectory through its junctions); equal offsets on both sides are an empty trajectory.  GGNNError otherwise.  Returns
    the boundary grains (global indices) of the trajectories that have nodes."""
    ng, nj = np.diff(grain_off), np.diff(joint_off)
    bad = np.flatnonzero((ng == 0) != (nj == 0))
    if bad.size:
        t = int(bad[0])
        raise _lib.GGNNError(f"traj_offsets: trajectory {t} has {int(ng[t])} grains and {int(nj[t])} junctions -- with "
                             "boundary='noflux' every non-empty trajectory owns at least one grain, its boundary grain, "
                             "and the junctions on its walls")
    return np.asarray(grain_off[:-1][ng > 0], np.int64)


class EnsembleSessions:
    """One TopologySession per trajectory of a disjoint-union graph: the reference's `Cmodel.update` sweeps,
    sorts and asserts over the WHOLE lists it is given (models.py:712-757, 730), so a union's events must be applied
    trajectory by trajectory, each on its own lists in its own (local) indices, and a refused update ends ONE trajectory.
    The union's lists are kept as the concatenation of the trajectories' lists in trajectory order."""

    def __init__(self, ei_jj: np.ndarray, ei_jg: np.ndarray, grain_offsets, joint_offsets):
        self.grain_off = np.asarray(grain_offsets, np.int64).reshape(-1)
        self.joint_off = np.asarray(joint_offsets, np.int64).reshape(-1)
        self.n_traj = self.grain_off.size - 1
        pp, pq = np.asarray(ei_jj, dtype=np.int64), np.asarray(ei_jg, dtype=np.int64)
        seg_pp = union_edge_segments(pp, self.joint_off, self.joint_off, "junction-junction list")
        seg_pq = union_edge_segments(pq, self.joint_off, self.grain_off, "junction-grain list")
        self.sessions = []
        for t in range(self.n_traj):
            j0, g0 = self.joint_off[t], self.grain_off[t]
            self.sessions.append(TopologySession(
                pp[:, seg_pp[t]:seg_pp[t + 1]] - j0, pq[:, seg_pq[t]:seg_pq[t + 1]] - np.array([[j0], [g0]], np.int64),
                int(self.joint_off[t + 1] - j0), int(self.grain_off[t + 1] - g0)))

    def close(self):
        for ses in self.sessions:
            ses.close()

    @property
    def n_pp(self):
        return sum(s.n_pp for s in self.sessions)

    @property
    def n_pq(self):
        return sum(s.n_pq for s in self.sessions)

    def segments(self):
        """Column offsets [n_traj + 1] of the trajectories' segments in the union's junction and junction-grain lists."""
        seg = lambda ns: np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        return seg([s.n_pp for s in self.sessions]), seg([s.n_pq for s in self.sessions])

    def local_lists(self, t: int):
        """Trajectory t's current lists in its own indices: {GJ, JG, JJ: int64 [2, n]}."""
        pp, pq, qp = self.sessions[t].export()
        return {GJ: qp, JG: pq, JJ: pp}

    def apply(self, x_joint: np.ndarray, y_joint: np.ndarray, y_grain_area: np.ndarray, edge_prob: np.ndarray,
              grain_area: np.ndarray, mask_grain: np.ndarray, mask_joint: np.ndarray, counts, ended, area_threshold: float,
              threshold: float, lists: Optional[np.ndarray] = None, skip_local_grain: Optional[int] = None):
        """One update of the union.  The arrays are the union's (x_joint [N_j, >= 8], y_joint [N_j, 2] fp32 C-contiguous,
        y_grain_area a float32 vector view [N_g] of the predicted area changes, edge_prob [n_pp] fp32, grain_area [N_g] the
        predicted areas, the int64 masks [N, 1] or [N]); every trajectory that has not `ended` and has a non-zero row of
        `counts` [n_traj, 2] gets its own update on its contiguous slices, in place: grain candidates = its live grains with
        grain_area < area_threshold, smallest first (stable), as test.py:418-420 on that trajectory alone, without the
        trajectory's grain `skip_local_grain` (local index; the no-flux boundary grain 0, dropped behind the sort as
        test.py:421-422 does; None: nobody).  A TopologyError ends at that trajectory: its slices and its session stay
        untouched.
        When a trajectory changed, the new union lists -- every trajectory's lists plus its node offsets, concatenated in
        trajectory order -- are written into `lists` (flat int64: [2, n_pp] then [2, n_pq]; default: a fresh array).
        Returns a dict: events (global grain ids: trajectory order, each trajectory's own order inside), switches
        ([S, 2] global junction ids), changed (trajectory indices), refused ({trajectory: message}), per_traj
        ({trajectory: (local events, local switches)}), n_pp, n_pq, lists (None when nothing changed)."""
        counts = np.asarray(counts).reshape(self.n_traj, 2)
        seg_pp, _ = self.segments()
        if edge_prob.shape[0] < seg_pp[-1]:
            raise ValueError(f"edge_prob needs one entry per junction edge of the union ({int(seg_pp[-1])})")
        mg, mj = mask_grain.reshape(-1), mask_joint.reshape(-1)
        if not (np.shares_memory(mg, mask_grain) and np.shares_memory(mj, mask_joint)):
            raise ValueError("the masks must be contiguous int64 arrays (they are rewritten in place)")
        events, switches, changed, refused, per_traj = [], [], [], {}, {}
        thr = np.float32(area_threshold)
        for t in range(self.n_traj):
            if (ended is not None and ended[t]) or not counts[t].any():
                continue
            j0, j1, g0, g1 = self.joint_off[t], self.joint_off[t + 1], self.grain_off[t], self.grain_off[t + 1]
            area = grain_area[g0:g1]
            ge = np.flatnonzero((mg[g0:g1] > 0) & (area < thr))
            ge = ge[np.argsort(area[ge], kind="stable")]
            if skip_local_grain is not None:
                ge = ge[ge != skip_local_grain]
            try:
                ev, sw = self.sessions[t].apply(x_joint[j0:j1], y_joint[j0:j1], y_grain_area[g0:g1], edge_prob[seg_pp[t]:seg_pp[t + 1]], ge,
                                                mg[g0:g1], mj[j0:j1], threshold)
            except TopologyError as err:
                refused[t] = str(err)
                continue
            if len(ev) == 0 and len(sw) == 0:
                continue   # (the device-side trigger was conservative: the update was the identity)
            changed.append(t)
            per_traj[t] = (ev, sw)
            events.append(ev + g0)
            switches.append(sw + j0)
        out = {"events": np.concatenate(events) if events else np.zeros(0, np.int64),
               "switches": np.concatenate(switches) if switches else np.zeros((0, 2), np.int64),
               "changed": changed, "refused": refused, "per_traj": per_traj, "n_pp": self.n_pp, "n_pq": self.n_pq,
               "lists": None}
        if changed:
            out["lists"] = self.export(lists)
        return out

    def export(self, lists: Optional[np.ndarray] = None):
        """The union's lists, global indices, trajectory order, into flat int64 `lists` ([2, n_pp] then [2, n_pq])."""
        n_pp, n_pq = self.n_pp, self.n_pq
        if lists is None:
            lists = np.empty(2 * (n_pp + n_pq), np.int64)
        pp, pq = lists[:2 * n_pp].reshape(2, n_pp), lists[2 * n_pp:2 * (n_pp + n_pq)].reshape(2, n_pq)
        seg_pp, seg_pq = self.segments()
        for t, ses in enumerate(self.sessions):
            ses.export(pp, pq, at=(seg_pp[t], seg_pq[t]))
            pp[:, seg_pp[t]:seg_pp[t + 1]] += self.joint_off[t]
            pq[0, seg_pq[t]:seg_pq[t + 1]] += self.joint_off[t]
            pq[1, seg_pq[t]:seg_pq[t + 1]] += self.grain_off[t]
        return lists


def update_topology(x_joint: np.ndarray, ei_jj: np.ndarray, ei_jg: np.ndarray, y_joint: np.ndarray,
                    y_grain: np.ndarray, edge_prob: np.ndarray, grain_event: Sequence[int],
                    mask_grain: np.ndarray, mask_joint: np.ndarray, threshold: float,
                    active_grains: Optional[np.ndarray] = None, active_joints: Optional[np.ndarray] = None):
    """One call of the reference's `Cmodel.update` (nucleation off).  `x_joint` [N_j, 8] fp32,
    `y_joint` [N_j, 2] fp32 and the masks are modified in place.  `edge_prob` = sigmoid of the
    classifier's `edge_event` logits, `grain_event` = grains below the area threshold, smallest
    first (test.py:418-420).  Returns (ei_jj, ei_jg, ei_gj, switching_list [S, 2], grain_event').
    Raises TopologyError when the lists are not a valid grain graph; the in-place arguments are then
    untouched (the library works on copies that are committed together)."""
    lib = _library()
    n_j, n_g = int(mask_joint.shape[0]), int(mask_grain.shape[0])
    for name, a, cols in (("x_joint", x_joint, None), ("y_joint", y_joint, 2)):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 2 or a.shape[0] != n_j \
                or (cols is not None and a.shape[1] != cols):
            raise ValueError(f"{name} must be a float32 numpy array [{n_j}, {cols or '>= 8'}]")
    if x_joint.shape[1] < 8:
        raise ValueError("x_joint needs the 8 junction features (columns 6, 7 = the displacement the events reset)")
    ge = np.ascontiguousarray(np.asarray(grain_event, dtype=np.int64).reshape(-1))
    n_pp, n_pq = int(ei_jj.shape[1]), int(ei_jg.shape[1])
    # (room for the result: a removed grain appends two columns and drops more than that)
    cap = n_pp + 2 * n_g + 2
    pp = np.empty((2, cap), dtype=np.int64)
    pp[:, :n_pp] = ei_jj
    pq = np.array(ei_jg, dtype=np.int64, order="C", copy=True)
    xj, yj = np.array(x_joint, order="C", copy=True), np.array(y_joint, order="C", copy=True)
    mg = np.ascontiguousarray(mask_grain.reshape(-1).astype(np.int64))
    mj = np.ascontiguousarray(mask_joint.reshape(-1).astype(np.int64))
    area = np.ascontiguousarray(np.asarray(y_grain, dtype=np.float32)[:, 0])
    prob = np.ascontiguousarray(np.asarray(edge_prob, dtype=np.float32).reshape(-1))
    if prob.shape[0] != n_pp or area.shape[0] != n_g:
        raise ValueError("edge_prob needs one entry per junction edge, y_grain one row per grain")
    act_g, act_j = _flags(active_grains, n_g), _flags(active_joints, n_j)
    switching = np.empty((max(n_pp, 1), 2), dtype=np.int64)
    extra = np.empty(n_g + 1, dtype=np.int64)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    A = _lib.TopologyArgs()
    A.pp, A.pq, A.n_pp, A.n_pq, A.pp_cap, A.pq_cap = p(pp), p(pq), n_pp, n_pq, cap, n_pq
    A.x_joint, A.y_joint, A.y_grain_area, A.edge_prob = p(xj), p(yj), p(area), p(prob)
    A.grain_event, A.mask_grain, A.mask_joint = p(ge), p(mg), p(mj)
    A.active_grain, A.active_joint, A.switching, A.events_extra = p(act_g), p(act_j), p(switching), p(extra)
    A.n_joint, A.n_grain, A.ldx, A.ldyg, A.n_grain_event = n_j, n_g, xj.shape[1], 1, ge.shape[0]
    A.switching_cap, A.extra_cap, A.threshold = switching.shape[0], extra.shape[0], float(threshold)
    rc = lib.ggnn_topology_update(ctypes.byref(A))
    if rc == _lib.GGNN_ETOPOLOGY:
        raise TopologyError(A.error.decode(errors="replace"))
    _lib.check(rc, "ggnn_topology_update")
    # commit: coordinates, displacement features and masks in place, the lists as new arrays
    x_joint[...] = xj
    y_joint[...] = yj
    mask_grain[...] = mg.reshape(mask_grain.shape)
    mask_joint[...] = mj.reshape(mask_joint.shape)
    new_pp = pp[:, :A.n_pp].copy()
    new_pq = pq[:, :A.n_pq].copy()
    events = np.concatenate([ge, extra[:A.n_extra]]) if A.n_extra else ge
    return new_pp, new_pq, new_pq[::-1].copy(), switching[:A.n_switching].copy(), events
