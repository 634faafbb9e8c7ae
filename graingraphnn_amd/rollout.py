"""Static-topology rollout driver: the hot loop of test.py:353-577 with everything that
runs per step kept on the device.

One step = Rmodel.forward + Cmodel.forward (test.py:382-383) + Rmodel.update (:400)
+ z advance and clamp (:401-407) + [grain-centre refresh, :468-478 + :556-559 via
graph.update(), when `refresh_centres=True`] + edge-length refresh (:562-575).  Grain-event /
edge-event topology surgery (Cmodel.update, :426) is host code outside this path; the topology
is therefore static here.

The whole step is 13 kernel launches (the regressor and the classifier share every launch of
their cells) with no host synchronisation and no allocation, so it can be replayed from a hipGraph
(`use_graph=True`) to remove launch overhead on small graphs.
"""
import os
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .backend import _WordArena, default_backend
from .engine import (Workspace, _check_x, graph_for, prepare_edges, run_encoder_decoder,
                     run_encoder_decoder_multi)
from .modules import _param_version, _param_version_sample
from .packing import EDGE_TYPES, NODE_TYPES, pack_classifier_heads, pack_regressor_heads

TRAIN_FRAMES = 120  # test.py:190
ET_JJ = ("joint", "connect", "joint")
JG = ("joint", "pull", "grain")
GJ = ("grain", "push", "joint")


def resolve_traj_offsets(own, passed, what):
    """The trajectory offsets an enable_* call works with on a no-flux rollout: `own` = the constructor's (grain, junction)
    offsets or None, `passed` = the call's argument ({'grain', 'joint'} dict, or -- enable_qoi -- the grain offsets alone) or
    None.  A no-flux union has ONE set of offsets, the constructor's (the forward graph and the boundary step are built from
    them): passed ones must be equal.  Returns (grain offsets, junction offsets) or None."""
    if own is None:
        if passed is not None:
            raise _lib.GGNNError(f"{what}(traj_offsets=...) with boundary='noflux': a noflux union takes its offsets at "
                                 "construction, GrainRollout(..., boundary='noflux', traj_offsets=...) -- every trajectory has "
                                 "a boundary grain of its own, which the forward graph and the boundary step must know")
        return None
    if passed is not None:
        try:
            same = (np.array_equal(np.asarray(passed["grain"], np.int64).reshape(-1), own[0])
                    and np.array_equal(np.asarray(passed["joint"], np.int64).reshape(-1), own[1])) if isinstance(passed, dict) \
                else np.array_equal(np.asarray(passed, np.int64).reshape(-1), own[0])
        except (KeyError, TypeError, ValueError):
            same = False
        if not same:
            raise _lib.GGNNError(f"{what}: traj_offsets differ from the ones this noflux rollout was built with")
    return own


def process_schedule_table(G=None, R=None, features=None):
    """The feature table of GrainRollout.set_process_schedule: (fp32 [n_rows, n_traj, 2], whether every trajectory shares
    one column).  From G and R ([n_rows] or [n_rows, n_traj]): 1 - G / 10 and R / 2 computed in float64 and rounded to fp32
    once -- the reference's assignment of a float64 scalar into a float32 tensor (test.py:378-379); or `features` ([n_rows, 2]
    or [n_rows, n_traj, 2]) as they are."""
    if (features is None) == (G is None and R is None) or (G is None) != (R is None):
        raise _lib.GGNNError("set_process_schedule takes G and R, or features=, not both and not neither")
    try:
        if features is None:
            g, r = np.asarray(G, np.float64), np.asarray(R, np.float64)
            if g.shape != r.shape or g.ndim not in (1, 2):
                raise _lib.GGNNError("G and R must have the same shape, [n_rows] or [n_rows, n_traj]")
            table = np.stack(((1.0 - g / 10.0).astype(np.float32), (r / 2.0).astype(np.float32)), axis=-1)
        else:
            table = np.asarray(features)
            if table.ndim not in (2, 3) or table.shape[-1] != 2:
                raise _lib.GGNNError("features must be [n_rows, 2] or [n_rows, n_traj, 2]")
            table = table.astype(np.float32)
    except (TypeError, ValueError) as exc:
        raise _lib.GGNNError(f"set_process_schedule: not a numeric array ({exc})") from exc
    shared = table.ndim == 2
    if shared:
        table = table[:, None, :]
    if table.shape[0] < 1 or table.shape[1] < 1:
        raise _lib.GGNNError("a process schedule needs at least one row and one trajectory")
    if not np.isfinite(table).all():
        raise _lib.GGNNError("the process schedule must be finite")
    return np.ascontiguousarray(table), shared


class _EdgeSets:
    """The per-edge buffers of a topology as views of ONE float32 allocation: two sets of edge lengths and two sets of edge
    records per edge type -- the two-stream step reads one set while its refresh writes the other
    (GrainRollout._enqueue_overlapped_step; GrainRollout._parity says which set is current) -- and the per-edge predictions
    `edge_event` and `edge`.  Sized for a `capacity` per edge type; `cut(E)` gives the views for lists of E <= capacity
    edges.  Every segment starts on a 16-byte boundary that does not depend on E: a topology that changes in place (the event
    loop) is re-cut and no address moves; a topology with buffers of its own is the same arrangement with the capacity equal
    to the size.
    zero: the allocation starts as zeros; otherwise nothing is initialised -- for lists the event loop installs: the refresh
    that follows an event writes every length, ggnn_edge_prepare / ggnn_step_refresh_prepare every record (zero padding
    included) before anything reads them.  (noflux: the records of a masked table end before the list's length, and the
    sweeps' clamps may read the rest as padding, which must be finite: always zeroed.)
    The views share the allocation's version counter: an in-place Python write into any of them shows in `buf._version`
    (GrainRollout._ensure_edge_records)."""

    def __init__(self, capacity, device, zero: bool):
        self.capacity = {et: int(capacity[et]) for et in EDGE_TYPES}
        count = _WordArena()
        self._segments(count)
        self.buf = (torch.zeros if zero else torch.empty)(count.at, dtype=torch.float32, device=device)
        self._lengths, self._records, self._edge_event, self._edge = self._segments(_WordArena(self.buf))

    def _segments(self, arena):
        """The segments in their one order, each for max(capacity, 1) edges; the records with the GGNN_UNIT_EDGES tail rows
        that pad the last unit's reads."""
        n = {et: max(c, 1) for et, c in self.capacity.items()}
        lengths = [{et: arena.take(n[et]) for et in EDGE_TYPES} for _ in range(2)]
        records = [{et: arena.take((self.capacity[et] + _lib.GGNN_UNIT_EDGES) * _lib.GGNN_EINFO_ROW) for et in EDGE_TYPES}
                   for _ in range(2)]
        return lengths, records, arena.take(n[ET_JJ]), arena.take(2 * n[ET_JJ])

    def cut(self, E):
        """-> ([lengths of set 0, of set 1]: {et: [E]}, [records of set 0, of set 1]: {et: [E + GGNN_UNIT_EDGES,
        GGNN_EINFO_ROW]}, edge_event [E_jj], edge [E_jj, 2]) for the list sizes `E` ({et: int})."""
        E = {et: int(E[et]) for et in EDGE_TYPES}
        if any(E[et] > self.capacity[et] for et in EDGE_TYPES):
            raise _lib.GGNNError(f"edge lists of {E} edges do not fit buffers of {self.capacity}")
        rows = {et: E[et] + _lib.GGNN_UNIT_EDGES for et in EDGE_TYPES}
        return ([{et: s[et][:E[et]] for et in EDGE_TYPES} for s in self._lengths],
                [{et: s[et][:rows[et] * _lib.GGNN_EINFO_ROW].view(rows[et], _lib.GGNN_EINFO_ROW) for et in EDGE_TYPES}
                 for s in self._records],
                self._edge_event[:E[ET_JJ]], self._edge[:2 * E[ET_JJ]].view(E[ET_JJ], 2))


class GrainRollout:
    JOINT_LAUNCH_MAX_JOINTS = 8000

    def __init__(self, rmodel, cmodel, x_dict: Dict[str, torch.Tensor], edge_index_dict,
                 edge_attr_dict, span: int, use_graph: bool = False, concurrent: bool = True,
                 refresh_centres: bool = False,
                 domain_factor: float = 1.0, domain_offset: Optional[torch.Tensor] = None,
                 joint_launches: Optional[bool] = None, boundary: str = "periodic", max_y: float = 1.0, traj_offsets=None):
        """refresh_centres: also recompute x_grain[:, :2] from the junction polygons every step,
        like the reference's traj.GNN_update + test.py:556-559 (default off = the static-geometry
        goldens).  domain_factor / domain_offset: `geometry_scaling` of test.py:310-312 when the
        domain was folded by scale_feature_patchs (offset [n_joint, 2], floor of the scaled xy).
        joint_launches: the regressor and the classifier see the same x, graph and edge geometry,
        so every stage of their cells can go out as ONE launch for both (13 launches per step);
        False = one set of launches per model, on two streams when `concurrent`.  Default (None):
        joint launches below JOINT_LAUNCH_MAX_JOINTS junctions, where a step is launch-bound
        (cfg2: 0.139 vs 0.162 ms per step); above it every kernel fills the chip by itself and the
        two-stream plan wins by overlapping kernels of different kinds -- one model's matrix-bound
        projection beside the other's memory-bound sweep (cfg3: 0.61 vs 0.66 ms per step).
        boundary: "periodic" (default) or "noflux" -- grain 0 is the boundary grain that wraps the domain (the reference's
        traj.BC == 'noflux', test.py:363-375, 418-422, 446-463): both forwards see the lists without grain 0's edges,
        grain 0 never takes part in events, and after every step's topology update the boundary step resets grain 0 and
        pins the junctions to [0,1] x [0,max_y] ("No-flux boundary").
        traj_offsets (noflux only): {'grain': [n_traj + 1], 'joint': [n_traj + 1]} -- the graph is a disjoint union of
        no-flux trajectories, trajectory t's boundary grain is its local grain 0 = global grain traj_offsets['grain'][t]
        (DESIGN.md 8e).  max_y, domain_factor: one box for the whole union; domain_offset: the trajectories' concatenated.
        enable_events / enable_qoi then use these offsets.  (Periodic unions pass their offsets to enable_events /
        enable_qoi.)"""
        if boundary not in ("periodic", "noflux"):
            raise _lib.GGNNError(f"boundary must be 'periodic' or 'noflux', got {boundary!r}")
        self.boundary, self.max_y = boundary, float(max_y)
        self.noflux = boundary == "noflux"
        self._traj = None                     # a no-flux union: its offsets (host and device) and boundary grains
        if traj_offsets is not None:
            if not self.noflux:
                raise _lib.GGNNError("GrainRollout(traj_offsets=...) belongs to boundary='noflux'; a periodic union passes "
                                     "its offsets to enable_events / enable_qoi")
            from .topology import check_noflux_union, check_traj_offsets
            og, oj = check_traj_offsets(traj_offsets, int(x_dict["grain"].shape[0]), int(x_dict["joint"].shape[0]))
            self._traj = {"grain": og, "joint": oj, "boundary_grains": check_noflux_union(og, oj)}
        self.be = default_backend()
        self.rmodel, self.cmodel = rmodel, cmodel
        self.x = {nt: x_dict[nt] for nt in NODE_TYPES}  # mutated in place, like the reference
        for nt in NODE_TYPES:
            _check_x(self.x[nt], rmodel.in_channels_dict[nt], nt)
            if not self.x[nt].is_contiguous():
                raise _lib.GGNNError("x_dict tensors must be contiguous")
        dev = self.x["joint"].device
        if self._traj is not None:
            self._traj["dev"] = (torch.from_numpy(self._traj["grain"]).to(dev), torch.from_numpy(self._traj["joint"]).to(dev))
        self.n_nodes = {nt: self.x[nt].size(0) for nt in NODE_TYPES}
        self.pred = {}                        # this step's predictions (run_events: one of its slots' dicts)
        # which buffers self.pred holds: 0 = the rollout's own; 1 + k = those of run_events' ring slot k; -(1 + k) = slot k's
        # per-node ones with the edge sets' own per-edge ones (a topology installed behind the slot's step: _cut_edge_sets)
        self._pred_at = 0
        self.mask = None                      # enable_events()
        self._cap = None                      # the in-place topology of the event loop (_enter_capacity_mode)
        self._spec = None                     # run_events' ring of slots and its block graphs (_spec_state)
        self._spec_quiet_blocks = 0           # run_events' quiet blocks in a row: the next block's size
        self._range_hit = False               # an fp16-range report of a step run_events committed (range_exceeded)
        self._evb = None                      # pinned staging of the event round trip (_event_buffers)
        self._topo = None                     # (session, its jj list, its jg list, their versions): _topology_session
        self._ens = None                      # enable_events(traj_offsets=...): the per-trajectory event layer (_enable_ensemble)
        # which of the two sets of edge lengths / edge records (_EdgeSets) and of the classifier's two copies of x is
        # current: an overlapped step reads set `_parity` and leaves the other one current
        self._parity = 0
        self._xcs = None                      # the classifier's two alternating copies of x (_overlap_buffers)
        self._xc_fresh = False
        self._graphs = None                   # run() / step() graphs per (steps, parity): _replay
        self._qoi = None                      # enable_qoi(): the accumulator of grain volumes and its launch constants
        self._sched = None                    # set_process_schedule(): the (G, R) table on the device and its counter word
        self._poly = None                     # enable_polygons(): the per-layer arena of grain polygons and its layer word
        self._invalidate_graphs(segments=True)   # step_events()' segment graphs: _segment_graphs, _graph_fwd, _graph_ref
        self._set_topology(edge_index_dict, edge_attr_dict)
        self.span = span
        # test.py:401-406 computes in fp32: z += fp32(span/121); clamp at fp32(120/121)
        self.dz = float(np.float32(span / (TRAIN_FRAMES + 1)))
        self.zmax = float(np.float32(TRAIN_FRAMES / (TRAIN_FRAMES + 1)))
        self.flags = torch.zeros(2, dtype=torch.int32, device=dev)
        self.packed = {}
        self.ws = {}
        self._pack_weights()
        # this rollout's own range-flag word (include/ggnn.h, OPERAND RANGE): the fused cells of its launches report here,
        # so that two rollouts on a device neither consume nor raise each other's reports
        self._range_word = torch.zeros(1, dtype=torch.int32, device=dev)
        for name in ("R", "C"):
            self.ws[name] = Workspace(*self.packed[name], self.n_nodes, dev)
            self.ws[name].range_flag = self._range_word
        nj, ng = self.n_nodes["joint"], self.n_nodes["grain"]
        f32 = dict(dtype=torch.float32, device=dev)
        self.pred.update({"joint": torch.empty(nj, 2, **f32), "grain": torch.empty(ng, 2, **f32),
                          "grain_area": torch.empty(ng, **f32)})
        self._tmp = torch.empty(nj, 8, **f32)
        # the regressor and the classifier are independent given (x, edge geometry): run them
        # on two HIP streams so one model's launch tails overlap the other's kernels
        if joint_launches is None:
            joint_launches = self.n_nodes["joint"] < self.JOINT_LAUNCH_MAX_JOINTS
        self.joint_launches = joint_launches
        self.concurrent = concurrent and not joint_launches
        self._side = (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)) if self.concurrent else None
        self.refresh_centres = refresh_centres
        self.domain_factor = float(domain_factor)
        self.domain_offset = None
        if (refresh_centres or self.noflux) and self.domain_factor > 1:
            if domain_offset is None:
                raise _lib.GGNNError("domain_factor > 1 needs domain_offset")
            self.domain_offset = domain_offset.to(dev, torch.float32).contiguous()
        self.steps_done = 0
        self.use_graph = use_graph

    @torch.no_grad()
    def set_process_parameters(self, G: float, R: float):
        """The reference's `--temporal` schedule (test.py:345-346, 376-378): thermal gradient G and pulling speed R
        of the step to come, written into the junction features (`x_joint[:, 3] = 1 - G / 10`, `x_joint[:, 4] = R / 2`)
        before the forwards.  The edge records of the next step carry the sources' features, so they are rebuilt: the
        in-place write bumps the tensor's version counter, which step() / run() check (`_ensure_edge_records`).  The
        values themselves (graph_trajectory.py:129-175, GR_seq_from_time) are the caller's: call this between steps.
        (A whole schedule, on the device and inside run() / run_events(): set_process_schedule.)"""
        if self._sched is not None:
            raise _lib.GGNNError("a process schedule is set (set_process_schedule): the steps write the parameters themselves; "
                                 "clear_process_schedule() first")
        self.x["joint"][:, 3] = 1.0 - float(G) / 10.0
        self.x["joint"][:, 4] = float(R) / 2.0

    # -- the (G, R) schedule on the device -----------------------------------------------------------------
    @torch.no_grad()
    def set_process_schedule(self, G=None, R=None, *, features=None, traj_offsets=None):
        """The reference's `--temporal` schedule (test.py:345-346, 376-379) as a table on the device: row r holds the
        thermal gradient and the pulling speed of the r-th step from this call, and from now on the tail of every step writes
        the row of the step to come into x_joint[:, 3:5] (one launch, ggnn_process_schedule, behind the boundary step, the
        centres and the QoI launch and in front of the launch that builds the next step's edge records) -- in step(), run(),
        step_events() and run_events(), eager and inside their hipGraphs: the row follows a counter word on the device.
        Row 0 is written now (an in-place write: the edge records are rebuilt before the next step); past the last row the
        last row holds, so after K steps x holds row min(K, n_rows - 1) (with n_rows = the number of steps: what the
        reference leaves).  Calling it again restarts at row 0 (a table of the same shape on the same offsets goes into
        the buffers of the one before: the captured graphs stay).
        G, R: arrays [n_rows] (every trajectory the same) or [n_rows, n_traj]; the features 1 - G / 10 and R / 2 are computed
        in float64 and rounded to fp32 once, as the reference's assignment does.  OR features: [n_rows, 2] or
        [n_rows, n_traj, 2], the fp32 feature values themselves.  Values must be finite.
        traj_offsets: for [.., n_traj] tables on a periodic union, {'joint': [n_traj + 1]} (or the {'grain', 'joint'} dict of
        enable_events); a no-flux union uses its constructor's offsets (None here, or equal ones).
        generator.reference_gr_schedule makes the reference's own (G, R) lists."""
        table, shared = process_schedule_table(G, R, features)
        off = self._schedule_offsets(traj_offsets)
        if shared:
            off = None   # one row for every junction: the launch needs no offsets
        elif off is None:
            if table.shape[1] != 1:
                raise _lib.GGNNError(f"a schedule of {table.shape[1]} trajectories needs traj_offsets={{'joint': [...]}} "
                                     "(a no-flux union: the constructor's)")
        elif off.size != table.shape[1] + 1:
            raise _lib.GGNNError(f"the schedule has {table.shape[1]} trajectories, the offsets {off.size - 1}")
        if off is not None and off.size == 2:
            off = None
        dev = self.x["joint"].device
        S = self._sched
        if S is not None and S["table_host"].shape == table.shape and (
                (off is None) == (S["offsets_host"] is None) and (off is None or np.array_equal(off, S["offsets_host"]))):
            # the same launch on the same buffers (another history of an ensemble sweep): new values, counter back to 0,
            # and every captured graph stays
            S["table_host"] = table
            S["table"].copy_(torch.from_numpy(table))
            S["home"]["flat"].zero_()
            S["at"] = None
        else:
            S = self._sched = {"name": "sched", "table_host": table, "table": torch.from_numpy(table).to(dev),
                               "offsets_host": off, "offsets": None if off is None else torch.from_numpy(off).to(dev),
                               "sync": torch.zeros(1, dtype=torch.int32, device=dev), "new": self._sched_state,
                               "home": self._sched_state(), "ring": None, "entries": None, "launched": 0, "at": None}
            # the launch list changed: every captured graph lacks (or has another) schedule launch
            self._invalidate_graphs(static=True, segments=True, blocks=True)
        # row 0, the step to come: an in-place write, seen by the version check of _ensure_edge_records
        row0 = S["table"][0]
        if off is not None:
            counts = torch.from_numpy(np.diff(off)).to(dev)
            row0 = torch.repeat_interleave(row0, counts, dim=0)
        self.x["joint"][:, 3:5] = row0
        self._einfo_fresh = False
        self._x_written_outside()

    def clear_process_schedule(self):
        """No schedule any more: the steps make the launches they made before set_process_schedule, x keeps the parameters
        it holds, and set_process_parameters works again."""
        if self._sched is not None:
            self._sched = None
            self._invalidate_graphs(static=True, segments=True, blocks=True)   # (every captured graph has the launch)

    def _invalidate_graphs(self, static=False, segments=False, blocks=False):
        """Drop captured hipGraphs, by family: `static` = those of run() / step() (_graphs: _replay), `segments` = those of
        step_events()' two segments (_segment_graphs, _graph_fwd, _graph_ref: _run_segment), `blocks` = those of run_events'
        blocks (_spec["graphs"]: _spec_launch) -- the last two with the list sizes they were captured at.  A graph holds
        the addresses of everything its launches read and write and the launch list of its moment, and its key (parity,
        slot) names neither: whatever replaces a buffer a graph may hold, or changes the launches of a step, drops the
        families that hold it here."""
        if static:
            self._graphs = None
        if segments:
            self._graph_fwd = self._graph_ref = None
            self._segment_graphs = {}
            if self._cap is not None:
                self._cap["captured"] = None
        if blocks and self._spec is not None:
            self._spec["graphs"], self._spec["captured"] = {}, None

    def _schedule_offsets(self, passed):
        """The junction offsets a schedule's trajectories are found with (int64 [n_traj + 1], host), or None: a no-flux
        union's own (passed ones must be equal), else the call's ({'joint': [...]} or the full dict)."""
        nj = self.n_nodes["joint"]
        if self.noflux:
            if self._traj is not None and isinstance(passed, dict) and "grain" not in passed:
                passed = dict(passed, grain=self._traj["grain"])
            own = resolve_traj_offsets(None if self._traj is None else (self._traj["grain"], self._traj["joint"]), passed,
                                       "set_process_schedule")
            return None if own is None else own[1]
        if passed is None:
            return None
        try:
            off = np.asarray(passed["joint"], dtype=np.int64).reshape(-1)
        except (KeyError, TypeError, ValueError, IndexError) as exc:
            raise _lib.GGNNError("set_process_schedule: traj_offsets must be {'joint': [n_traj + 1]}") from exc
        if off.size < 2 or off[0] != 0 or off[-1] != nj or (np.diff(off) < 0).any():
            raise _lib.GGNNError("traj_offsets['joint'] must rise from 0 to the number of junctions")
        return off

    def _sched_state(self):
        """One counter word of the schedule (`flat`: what a state is copied by, as the QoI accumulator's)."""
        return {"flat": torch.zeros(1, dtype=torch.int32, device=self.x["joint"].device)}

    def _enqueue_schedule(self, slot=None):
        """The parameters of the step to come (off unless set_process_schedule was called): counter and row on the rollout's
        own word in place, or -- a ring `slot` of the speculative event loop -- from the word of the slot before to the
        slot's own."""
        S = self._sched
        if S is None:
            return
        src = dst = S["home"]
        if slot is not None:
            src, dst = S["ring"][(slot - 1) % len(S["ring"])], S["ring"][slot]
        self.be.process_schedule(self.x["joint"], S["table"], S["offsets"], src["flat"], dst["flat"], S["sync"])

    def _pack_weights(self):
        """Fused device weights of both models, and the parameter versions they were packed from."""
        self._wver = (_param_version(self.rmodel), _param_version(self.cmodel))
        self._wver_sample = (_param_version_sample(self.rmodel), _param_version_sample(self.cmodel))
        for name, m in (("R", self.rmodel), ("C", self.cmodel)):
            self.packed[name] = (m.gclstm_encoder.cell_list[0].packed(True),
                                 m.gclstm_decoder.cell_list[0].packed(False, m._live_out))
        self.w_reg = pack_regressor_heads(self.rmodel.linear)
        self.w_cls = pack_classifier_heads(self.cmodel.lin1, self.cmodel.lin2)

    def refresh_weights(self, force: bool = False, sample: bool = False):
        """Re-pack the weights and drop the captured hipGraphs (which hold the old buffers'
        addresses) if a parameter of either model was updated, moved or replaced since they were
        packed (load_state_dict, an optimizer step, .to()).  Checked on every run() / run_events() call and
        on every 16th step() / step_events() call (the check walks 568 tensors, ~0.15 ms: a seventh of an
        eventful step); the step_events() calls between look at a sample of the tensors (`sample`: every 24th --
        what changes a model changes all of it); call it directly after changing single parameters
        between two step() / step_events() calls."""
        if sample and not force:
            now = (_param_version_sample(self.rmodel), _param_version_sample(self.cmodel))
            if now == self._wver_sample:
                return
        if force or self._wver != (_param_version(self.rmodel), _param_version(self.cmodel)):
            self._pack_weights()
            self._invalidate_graphs(static=True, segments=True)
            self._spec = None   # (run_events' captured blocks hold the old buffers' addresses too)

    def _set_topology(self, edge_index_dict, edge_attr_dict=None, lasting=True, trusted=False):
        """(Re)build everything that depends on the edge lists: CSR + unit tables, the edge-length
        buffers (refreshed in place every step), the per-edge geometry records and the per-edge
        outputs.  Called once at construction and after every topological event (`trusted`: lists the
        library's own update produced -- no range check, no read-back)."""
        dev = self.x["joint"].device
        if self._cap is not None:
            if trusted and edge_attr_dict is None and all(edge_index_dict[et].size(1) <= self._cap["cap"][et] for et in EDGE_TYPES):
                return self._install_topology_in_place(edge_index_dict)
            self._cap = None   # (a caller's own topology, or one that grew: back to buffers of its own)
        self.edge_index = {et: edge_index_dict[et] for et in EDGE_TYPES}
        self.graph = graph_for(self.be, self.edge_index, self.n_nodes, trusted, self.boundary, self._traj_grain_dev())
        # buffers of its own: edge sets whose capacity is the size.  Lists the event loop installs (every step, on the
        # reference's trajectories) are written before they are read: nothing to initialise (_EdgeSets)
        E = {et: self.edge_index[et].size(1) for et in EDGE_TYPES}
        self._sets = _EdgeSets(E, dev, zero=self.noflux or not (trusted and edge_attr_dict is None))
        self._cut_edge_sets(E)
        if edge_attr_dict is not None:
            for et in EDGE_TYPES:
                self.edge_attr[et].copy_(edge_attr_dict[et].detach().reshape(-1))
        # new CSR tables and new per-edge buffers: whatever was captured holds the old ones
        self._invalidate_graphs(static=True, segments=True, blocks=True)

    def _cut_edge_sets(self, E):
        """The views of the edge sets for lists of `E` edges (_EdgeSets.cut) become the rollout's per-edge tensors.  The
        records are to be prepared and the version counters to be read again; the classifier's copies of x keep their
        buffers (the node sets never change) but no longer mirror x."""
        self._ea, self._recs, edge_event, edge = self._sets.cut(E)
        if self._pred_at > 0:   # (a ring slot's dict, run_events: the slot keeps its own per-edge predictions)
            self.pred, self._pred_at = dict(self.pred), -self._pred_at
        self.pred["edge_event"], self.pred["edge"] = edge_event, edge
        # which of the two sets is the current one follows the speculative loop's slot parity while its ring lives
        # (run_events' graphs alternate the sets by slot: _spec_state); otherwise the first
        self._parity = 0 if self._spec is None else self._spec["cur"] & 1
        self._einfo_fresh = False   # True: self.einfo already holds the records of the step to come
        self._x_written_outside()
        self._seen = None

    @property
    def edge_attr(self):
        """The current edge lengths, {edge type: [E]}: refreshed by every step, and the caller's to write in place."""
        return self._ea[self._parity]

    @property
    def einfo(self):
        """The current set of edge records, {edge type: [E + GGNN_UNIT_EDGES, GGNN_EINFO_ROW]}."""
        return self._recs[self._parity]

    # -- a topology that changes IN PLACE (event mode) ---------------------------------------------------------------------
    def _enter_capacity_mode(self):
        """enable_events(): the edge lists, the CSR tables and every per-edge buffer move into allocations of the CURRENT
        lists' size -- the capacity: grain eliminations only remove edges, neighbour switches keep their number -- and stay
        there: an event rewrites them in place (_install_topology_in_place), the per-edge kernels read the number of edges from
        device memory (CSR.E_dev), and the hipGraphs of step_events()' two segments keep replaying across events (SURVEY 8
        f-2: "keep the device rollout running between events"; round 5 dropped every graph with the topology and ran the
        steps around an event eagerly).  The fused cells need nothing: their grids follow the node sets, their edge windows
        come from the rebuilt row pointers, and an edge count that is too large only widens a clamp onto stale, valid entries."""
        be, dev = self.be, self.x["joint"].device
        if not hasattr(be, "csr_in_place") or os.environ.get("GGNN_EVENT_GRAPHS", "1") == "0":
            self._cap = None
            return
        cap = {et: int(self.edge_index[et].size(1)) for et in EDGE_TYPES}
        old_ea = {et: self.edge_attr[et] for et in EDGE_TYPES}
        old_ei = {et: self.edge_index[et] for et in EDGE_TYPES}
        self._sets = _EdgeSets(cap, dev, zero=self.noflux)
        self._cap = {
            "cap": cap,
            "lists": {et: torch.empty(2 * max(cap[et], 1), dtype=torch.int64, device=dev) for et in EDGE_TYPES},
            "csr": self._csr_in_place(be, cap, dev),
            "counts": torch.zeros(len(EDGE_TYPES), dtype=torch.int64, device=dev),
            "counts_host": torch.zeros(len(EDGE_TYPES), dtype=torch.int64).pin_memory(),
            "captured": None,   # the smallest list sizes the segment graphs were captured at (_run_segment)
        }
        self._install_topology_in_place(old_ei)
        for et in EDGE_TYPES:
            self.edge_attr[et].copy_(old_ea[et])
        self._invalidate_graphs(segments=True, blocks=True)   # (what was captured holds the buffers of before)

    def _install_topology_in_place(self, edge_index_dict):
        """The lists of `edge_index_dict` (device tensors, or already views of the list buffers) become the topology: copied
        into the list buffers, their sizes into the device-side counts, the CSR tables rebuilt inside the arena, the per-edge
        tensors re-cut as views of the same allocations.  No address changes: the segment graphs stay."""
        C = self._cap
        E = {et: int(edge_index_dict[et].size(1)) for et in EDGE_TYPES}
        self.edge_index = {}
        for k, et in enumerate(EDGE_TYPES):
            dst = C["lists"][et][:2 * E[et]].view(2, E[et])
            src = edge_index_dict[et]
            if src.data_ptr() != dst.data_ptr():
                dst.copy_(src, non_blocking=True)
            self.edge_index[et] = dst
            C["counts_host"][k] = E[et]
        C["counts"].copy_(C["counts_host"], non_blocking=True)
        counts = {et: C["counts"][k:k + 1] for k, et in enumerate(EDGE_TYPES)}
        from .engine import GraphCSR
        self.graph = GraphCSR(self.be, self.edge_index, self.n_nodes, trusted=True, into=C["csr"], counts=counts,
                              boundary=self.boundary, traj_grain_off=self._traj_grain_dev())
        self._cut_edge_sets(E)
        # run() / step() graphs hold the sizes of their moment in their launches; a segment or block graph reads them from
        # the device: it stays valid while nothing has grown since it was captured
        grown = self._outgrown(C["captured"])
        self._invalidate_graphs(static=True, segments=grown, blocks=grown)

    def _x_written_outside(self):
        """x was (or is about to be) advanced by something other than the overlapped two-stream step / the speculative
        event step: their mirrors of x (the copies the classifier's forward reads) are stale."""
        self._xc_fresh = False
        if self._spec is not None:
            self._spec["xs_valid"] = None

    def _outgrown(self, captured):
        """Whether a list is longer now than the smallest sizes `captured` (or None) that a set of graphs was captured at:
        graphs on the in-place topology stay valid only while none has grown."""
        return captured is not None and any(int(self.edge_index[et].size(1)) > captured[et] for et in EDGE_TYPES)

    def _smallest_sizes(self, captured):
        """`captured` (the smallest list sizes a set of graphs was captured at, or None) with a capture at the current sizes."""
        now = {et: int(self.edge_index[et].size(1)) for et in EDGE_TYPES}
        return now if captured is None else {et: min(now[et], captured[et]) for et in EDGE_TYPES}

    # -- no-flux boundary ------------------------------------------------------------------
    def _csr_in_place(self, be, cap, dev):
        """The in-place CSR tables of the event loop: the three edge types, and for the no-flux boundary the forward's
        masked grain tables plus the full joint->grain table (engine.GraphCSR)."""
        shapes = [(cap[et], self.n_nodes[et[0]], self.n_nodes[et[-1]]) for et in EDGE_TYPES]
        if not self.noflux:
            return be.csr_in_place(shapes, dev)
        from .engine import NOFLUX_MASKS, noflux_unions
        union = {} if self._traj is None else {"unions": noflux_unions(self._traj_grain_dev())}
        return be.csr_in_place(shapes + [(cap[JG], self.n_nodes["joint"], self.n_nodes["grain"])], dev,
                               [NOFLUX_MASKS[et] for et in EDGE_TYPES] + [None], **union)

    def _traj_grain_dev(self):
        """A no-flux union's grain offsets on the device (every trajectory's first grain is a boundary grain), or None."""
        return None if self._traj is None else self._traj["dev"][0]

    def _enqueue_boundary(self, joints_before=None):
        """test.py:446-463 (noflux only): grain 0 reset, its junctions onto the walls, every junction into the domain; a
        union: every trajectory's boundary grain and its junctions, in the same launch."""
        if self.noflux:
            union = {} if self._traj is None else {"traj_offsets": self._traj["dev"]}
            self.be.noflux_boundary(self.graph.csr_full[JG], self.x["joint"], self.x["grain"], self.domain_factor,
                                    self.domain_offset, self.max_y, joints_before, **union)

    def _enqueue_centres(self, centres_before=None):
        """graph.update()'s region centres + test.py:556-559 (refresh_centres); noflux: from the full joint->grain table,
        without min-image chaining."""
        self.be.grain_centres(self.graph.csr_full[JG], self.x["joint"], self.x["grain"], self.domain_factor,
                              self.domain_offset, centres_before=centres_before, boundary=self.boundary)

    # -- quantities of interest: grain volumes and size statistics (graph_trajectory.py:1042-1051, 221-256) -----------
    def enable_qoi(self, patch_size, mesh_size, ini_height, final_height, frames=None, capacity=None, area0=None,
                   history=True, traj_offsets=None):
        """Accumulate, from now on and on the device, what the reference's rollout records at every frame and integrates at
        its end: the normalised live-grain areas and scaled excess volumes (GNN_update's "qoi", graph_trajectory.py:1042-1051),
        their trapezoid integral over the layers (volume('graph'), :221-242) and, in qoi(), the equivalent diameters with
        d_mu, d_std and the histogram (:244-256).  One launch per step (ggnn_qoi_accumulate, include/ggnn.h) behind the
        step's topology update and boundary step, in step() / run() / step_events() / run_events() and inside their
        hipGraphs.  Layer 0 -- the state as it is now -- is computed at once.
        patch_size, mesh_size, ini_height, final_height: the trajectory object's (40, 0.08, 2, 50 by default there);
        frames: test.py:307, int((final_height - ini_height) / 0.4) + 1; capacity: the number of layers a kept history has
        room for beyond layer 0 (default: the steps the frames allow, (frames - 1) // span); area0 [n_grain]: layer 0's
        areas when they are not the formula's (the reference keeps its rasterised pixel counts there, test.py:340);
        history=False keeps no volume_traj; traj_offsets: the first grain of every trajectory of a disjoint-union graph and
        the total, [n_traj + 1] (default: one trajectory; a no-flux union: the constructor's, and nothing else)."""
        dev, ng = self.x["grain"].device, self.n_nodes["grain"]
        if self._traj is not None:
            traj_offsets = resolve_traj_offsets((self._traj["grain"], self._traj["joint"]), traj_offsets, "enable_qoi")[0]
        if frames is None:
            frames = int((final_height - ini_height) / 0.4) + 1   # test.py:191, 307
        if not (mesh_size > 0 and patch_size > 0 and frames > 1):
            raise _lib.GGNNError("enable_qoi: mesh_size and patch_size must be positive, frames at least 2")
        if capacity is None:
            capacity = (int(frames) - 1) // self.span
        off = np.asarray([0, ng] if traj_offsets is None else traj_offsets, dtype=np.int64).reshape(-1)
        if off.size < 2 or off[0] != 0 or off[-1] != ng or (np.diff(off) < 0).any():
            raise _lib.GGNNError("traj_offsets must rise from 0 to the number of grains")
        delta_h = self.span * (final_height - ini_height) / mesh_size / (frames - 1)
        f32 = dict(dtype=torch.float32, device=dev)
        Q = self._qoi = {
            "name": "qoi", "new": self._qoi_state,
            "const": (self.domain_factor, patch_size / mesh_size + 1, delta_h), "mesh_size": float(mesh_size),
            "capacity": int(capacity), "offsets_host": off, "offsets": torch.from_numpy(off).to(dev),
            "V0": torch.empty(ng, **f32), "home": self._qoi_state(), "words": torch.zeros(2, dtype=torch.int32, device=dev),
            "history": torch.zeros(int(capacity) + 1, ng, **f32) if history else None,
            "area_sum": torch.empty(off.size - 1, **f32),
            "ring": None, "entries": None, "launched": 0, "at": None}
        if area0 is not None:
            area0 = torch.as_tensor(area0).to(dev, torch.float32).contiguous().view(-1)
            if area0.numel() != ng:
                raise _lib.GGNNError("area0 must have one entry per grain")
        self._invalidate_graphs(static=True, segments=True, blocks=True)   # (graphs captured so far lack the launch)
        self._enqueue_qoi(init=True, area0=area0)

    def _qoi_state(self):
        """One accumulator: a_k, T_k, e_k per grain and the layer counter, in ONE allocation (a state is copied in one
        copy).  The rollout's own (`home`) is advanced in place; run_events keeps one per ring slot."""
        ng, dev = self.n_nodes["grain"], self.x["grain"].device
        n4 = (ng + 3) & ~3
        flat = torch.zeros(3 * n4 + 4, dtype=torch.float32, device=dev)
        return {"flat": flat, "a": flat[:ng], "T": flat[n4:n4 + ng], "e": flat[2 * n4:2 * n4 + ng],
                "layer": flat[3 * n4:].view(torch.int32)[:1]}

    def _enqueue_qoi(self, slot=None, init=False, area0=None):
        """This step's layer (off unless enable_qoi was called): on the rollout's own accumulator in place, or -- a ring
        `slot` of the speculative event loop -- from the slot before to the slot's own."""
        Q = self._qoi
        if Q is None:
            return
        src = dst = Q["home"]
        if slot is not None:
            src, dst = Q["ring"][(slot - 1) % len(Q["ring"])], Q["ring"][slot]
        self.be.qoi_accumulate(self.x["grain"], self._live_grain if self.mask is not None else None, Q["offsets"],
                               Q["const"], src, dst, Q["V0"], Q["words"][:1], Q["words"][1:], Q["history"], Q["capacity"],
                               Q["area_sum"], init=init, area0=area0)

    # -- the layers' grain polygons (graph.update(), graph_datastruct.py:654-721) ---------------------------
    def enable_polygons(self, capacity=None, traj_offsets=None, positions=False):
        """Record, from now on and on the device, every layer's grain polygons: what the reference's rollout leaves in
        traj.regions / region_coors / region_center after traj.GNN_update (test.py:468-478) -- per grain the junctions of its
        row of the joint->grain table, unwrapped, ordered counter-clockwise round their mean, with the mean and the shoelace
        area.  One launch per step (ggnn_grain_polygons, include/ggnn.h) behind the boundary step and the centre refresh, in
        step() / run() / step_events() / run_events() and inside their hipGraphs; the launch only reads the state.  Layer 0
        -- the state as it is now -- is recorded at once.
        capacity: the number of layers the arena has room for beyond layer 0 (default: enable_qoi's, when it was called
        before; otherwise required).  The arena's rows have the size of the table as it is now: eliminations only shrink it.
        traj_offsets: {'grain': [n_traj + 1], 'joint': [n_traj + 1]} of a disjoint-union graph, for polygons(traj=t)
        (default: the constructor's of a no-flux union, or enable_events').
        positions: also keep what every layer's launch read -- the table's columns and the junctions in the global frame
        (ggnn_polygon_inputs, one more launch per step in front of the polygon launch) -- which interp_polygons and
        grain_volume(interp_frames > 0) blend between layers.  Off: the step's launches are what they are
        without it."""
        if capacity is None:
            if self._qoi is None:
                raise _lib.GGNNError("enable_polygons: capacity (the number of steps to record) is required unless enable_qoi "
                                     "was called before")
            capacity = self._qoi["capacity"]
        if int(capacity) < 0:
            raise _lib.GGNNError("enable_polygons: capacity must not be negative")
        offsets = None
        if self._traj is not None:
            resolve_traj_offsets((self._traj["grain"], self._traj["joint"]), traj_offsets, "enable_polygons")
        elif traj_offsets is not None:
            from .topology import check_traj_offsets
            offsets = check_traj_offsets(traj_offsets, self.n_nodes["grain"], self.n_nodes["joint"])
        dev, ng = self.x["grain"].device, self.n_nodes["grain"]
        self._poly = {
            "name": "poly", "new": self._poly_state, "capacity": int(capacity), "offsets": offsets,
            "arena": self.be.polygon_arena(ng, int(self.graph.edge_index[JG].size(1)), int(capacity), dev),
            "inputs": self.be.polygon_inputs_arena(self.n_nodes["joint"], int(self.graph.edge_index[JG].size(1)), int(capacity),
                                                   dev) if positions else None,
            "home": self._poly_state(), "words": torch.zeros(2, dtype=torch.int32, device=dev),
            "ring": None, "entries": None, "launched": 0, "at": None}
        self._invalidate_graphs(static=True, segments=True, blocks=True)   # (graphs captured so far lack the launch)
        self._enqueue_polygons(init=True)

    def _poly_state(self):
        """One counter word of the recorder: the layer written last (`flat`: what a state is copied by)."""
        flat = torch.zeros(1, dtype=torch.int32, device=self.x["joint"].device)
        return {"flat": flat, "layer": flat}

    def _enqueue_polygons(self, slot=None, init=False):
        """This step's layer of polygons (off unless enable_polygons was called): counted on the rollout's own word in
        place, or -- a ring `slot` of the speculative event loop -- from the word of the slot before to the slot's own.
        The arena is one: a voided step's row is written again by the step that stands."""
        P = self._poly
        if P is None:
            return
        if self.graph.edge_index[JG].size(1) > P["arena"]["joint_sorted"].size(1):
            raise _lib.GGNNError("the joint->grain list has grown beyond the rows enable_polygons allocated: call it again")
        src = dst = P["home"]
        if slot is not None:
            src, dst = P["ring"][(slot - 1) % len(P["ring"])], P["ring"][slot]
        if P.get("inputs") is not None:   # (the same word, read before the polygon launch advances it)
            self.be.polygon_inputs(self.graph.csr_full[JG], self.x["joint"], P["inputs"], self.domain_factor,
                                   self.domain_offset, layer_in=None if init else src["layer"])
        self.be.grain_polygons(self.graph.csr_full[JG], self.x["joint"], P["arena"], self.domain_factor, self.domain_offset,
                               boundary=self.boundary, traj_grain_off=self._traj_grain_dev(),
                               layer_in=None if init else src["layer"], layer_out=dst["layer"], sync_word=P["words"][:1],
                               flags=P["words"][1:])

    def _polygon_offsets(self):
        """(grain offsets, junction offsets) of the union polygons(traj=t) slices, host int64, or None."""
        if self._poly["offsets"] is not None:
            return self._poly["offsets"]
        if self._traj is not None:
            return self._traj["grain"], self._traj["joint"]
        if self._ens is not None:
            ens = self._ens["sessions"]
            return np.asarray(ens.grain_off, np.int64), np.asarray(ens.joint_off, np.int64)
        return None

    def polygons(self, layer=None, traj=None):
        """The recorded polygons of one layer (one synchronisation): the last one, or `layer` = k (0 = the state
        enable_polygons found).  Device tensors in the layout of the layer's joint->grain table: `rowptr` int32 [n + 1] (grain
        g owns entries rowptr[g]:rowptr[g + 1]), `sides` [n], `joint_sorted` int32 [E] (the junctions counter-clockwise from
        angle 0 round the centre; a no-flux boundary grain clockwise), `xy_sorted` fp32 [E, 2] (their unwrapped
        coordinates), `centre` fp32 [n, 2] (unfolded), `area` fp32 [n] (shoelace, negative for a reversed grain); and
        `layer`, `layers` (steps recorded).  traj=t (a union with known offsets): that trajectory's grains alone, rowptr
        from 0 and junction ids local to the trajectory.  With enable_events(traj_offsets=...) `layers` is an array without
        `traj`, and a trajectory that ended (trajectory_states) reports the layers up to its last completed step.  With
        enable_polygons(positions=True) also `col` int32 [E] (the table's columns as the layer's launch read them, local with
        traj=t) and `joint_xy` fp32 [n_joint, 2] (the junctions in the global frame; traj=t: the trajectory's).  Raises
        when a layer went beyond the capacity, or `layer` was not recorded."""
        P = self._poly
        if P is None:
            raise _lib.GGNNError("call enable_polygons(...) first")
        self._carry_home()
        A, ng, cap = P["arena"], self.n_nodes["grain"], P["capacity"]
        g0, g1, j0, j1 = 0, ng, 0, self.n_nodes["joint"]
        if traj is not None:
            off = self._polygon_offsets()
            if off is None:
                raise _lib.GGNNError("polygons(traj=...) needs the union's offsets: enable_polygons(traj_offsets=...)")
            t = int(traj)
            if not 0 <= t < len(off[0]) - 1:
                raise _lib.GGNNError(f"no trajectory {traj}: the union has {len(off[0]) - 1}")
            g0, g1, j0, j1 = int(off[0][t]), int(off[0][t + 1]), int(off[1][t]), int(off[1][t + 1])
        ended = []   # (trajectory, the layer word of its last completed step)
        if self._ens is not None:
            ended = [(t_, sn["poly_layer"]) for t_, sn in enumerate(self._ens["snapshot"])
                     if sn is not None and sn.get("poly_layer") is not None]
        count = next((w for t_, w in ended if traj is not None and t_ == int(traj)), P["home"]["layer"])
        if layer is None:
            row = A["rowptr"].index_select(0, count.long().clamp(0, cap))[0]
        else:
            if not 0 <= int(layer) <= cap:
                raise _lib.GGNNError(f"layer {layer} is outside the arena's 0..{cap}")
            row = A["rowptr"][int(layer)]
        marks = row[torch.tensor([g0, g1, ng], device=row.device)]
        words = torch.cat([P["home"]["layer"], P["words"][1:], count, marks] + [w for _, w in ended]).cpu().tolist()
        if words[1] & _lib.GGNN_FLAG_POLYGON_OVERFLOW:
            raise _lib.GGNNError(f"the polygon arena has room for {cap} layers, {words[0]} were recorded: "
                                 "enable_polygons(capacity=...)")
        layers = words[2]
        k = layers if layer is None else int(layer)
        if k > layers:
            raise _lib.GGNNError(f"layer {k} has not been recorded: {layers} layers so far")
        e0, e1 = words[3], words[4]
        res = {"layer": k, "layers": layers, "rowptr": A["rowptr"][k, g0:g1 + 1] - e0,
               "joint_sorted": A["joint_sorted"][k, e0:e1] - j0, "xy_sorted": A["xy_sorted"][k, e0:e1],
               "centre": A["centre"][k, g0:g1], "area": A["area"][k, g0:g1]}
        res["sides"] = res["rowptr"][1:] - res["rowptr"][:-1]
        if P.get("inputs") is not None:
            res["col"], res["joint_xy"] = P["inputs"]["col"][k, e0:e1] - j0, P["inputs"]["joint_xy"][k, j0:j1]
        if self._ens is not None and traj is None:   # per trajectory of the event layer: an ended one stopped counting
            per = np.full(self._ens["n_traj"], layers, dtype=np.int64)
            for i, (t_, _) in enumerate(ended):
                per[t_] = words[6 + i]
            res["layers"] = per
        return res

    # -- in-between layers and the 3-D volume (test.py:494-528, pv_3Dview.py:150-192) ---------------------------
    def _interp_arena(self, jobs, traj):
        """The records of `jobs` = [(layer, coefficient)] as a polygon arena of len(jobs) rows (one synchronisation: the
        layers recorded so far, of `traj` where it ended early)."""
        recorded = int(np.max(self.polygons(None, traj)["layers"]))
        P = self._poly
        if P.get("inputs") is None:
            raise _lib.GGNNError("in-between layers need the recorded positions: enable_polygons(..., positions=True)")
        if recorded < 1:
            raise _lib.GGNNError("an in-between layer needs two recorded layers: take a step first")
        return self.be.interp_polygons(P["arena"], P["inputs"], jobs, recorded, self.boundary, self.max_y,
                                       self._traj_grain_dev())

    def interp_polygons(self, layer, coeff, traj=None):
        """The polygon record of the in-between layer coeff * layer + (1 - coeff) * (layer - 1), as the reference's
        --interp_frames builds it (test.py:494-528): junction positions blended, the topology of the nearer layer (`layer`'s
        for coeff > 0.5), no-flux junctions of the boundary grain moved to the nearest wall and all clamped to the box; then
        the rule of polygons() (include/ggnn.h, ggnn_interp_polygons).  Periodic positions are blended along the short way
        across the walls and are not snapped.  Returns the dict polygons() returns (`layer`: the layer whose topology it
        has; no `col` / `joint_xy`).  Needs enable_polygons(positions=True).  On demand, on the current stream."""
        whole = self.polygons(None, traj)
        arena = self._interp_arena([(layer, coeff)], traj)
        top = int(layer) if float(coeff) > 0.5 else int(layer) - 1
        g0, g1, j0 = 0, self.n_nodes["grain"], 0
        if traj is not None:
            off = self._polygon_offsets()
            g0, g1, j0 = int(off[0][int(traj)]), int(off[0][int(traj) + 1]), int(off[1][int(traj)])
        e0, e1 = (int(v) for v in arena["rowptr"][0, [g0, g1]].cpu())
        res = {"layer": top, "layers": whole["layers"], "rowptr": arena["rowptr"][0, g0:g1 + 1] - e0,
               "joint_sorted": arena["joint_sorted"][0, e0:e1] - j0, "xy_sorted": arena["xy_sorted"][0, e0:e1],
               "centre": arena["centre"][0, g0:g1], "area": arena["area"][0, g0:g1]}
        res["sides"] = res["rowptr"][1:] - res["rowptr"][:-1]
        return res

    def grain_volume(self, size, interp_frames=0, layers=None, traj=None, corner_grains=None, out=None):
        """The 3-D grain-ID volume of the rollout, int32 [nz, ny, nx] on the device: the reference's `alpha_field_list`
        stacked (pv_3Dview.py:150-192) -- layer 0, then for every later layer its `interp_frames` in-between images with
        coefficient (1 + i) / (1 + interp_frames), i = 0 .., then the layer's own (test.py:494-528).  In C order this is
        np.stack(alpha_field_list, axis=2).ravel(order='F'): vtkio.write_vtk needs no transpose.  layers: the recorded
        layers to take (default: all; in-between frames lie between a layer and the recorded one before it).  One
        interpolation call and one rasteriser launch per 256 images; interp_frames=0 is grain_images(size, layers)."""
        k_in = int(interp_frames)
        if k_in < 0:
            raise _lib.GGNNError("interp_frames must not be negative")
        if k_in == 0:
            return self.grain_images(size, layers, traj, corner_grains, out)
        if self._poly is not None and self._poly.get("inputs") is None:
            raise _lib.GGNNError("in-between layers need the recorded positions: enable_polygons(..., positions=True)")
        recorded = int(np.max(self.polygons(None, traj)["layers"]))
        layers = list(range(recorded + 1)) if layers is None else [int(k) for k in layers]
        for k in layers:
            if not 0 <= k <= recorded:
                raise _lib.GGNNError(f"layer {k} has not been recorded: {recorded} layers so far")
        jobs, rows = [], []   # rows: (is a job, its index) in the volume's order
        for k in layers:
            if k > 0:
                for i in range(k_in):
                    rows.append((True, len(jobs)))
                    jobs.append((k, (1 + i) / (1 + k_in)))
            rows.append((False, k))
        if not jobs:
            return self.grain_images(size, layers, traj, corner_grains, out)
        made, A = self._interp_arena(jobs, traj), self._poly["arena"]
        # one arena for the rasteriser: the interpolated rows, then the recorded ones that are drawn
        kept = sorted({k for is_job, k in rows if not is_job})
        at = {k: len(jobs) + i for i, k in enumerate(kept)}
        idx = torch.tensor(kept, device=A["rowptr"].device)
        both = {name: torch.cat([made[name], A[name].index_select(0, idx)]) for name in ("rowptr", "xy_sorted")}
        order = [i if is_job else at[i] for is_job, i in rows]
        return self.be.rasterize_polygons(both, size, order, self.boundary, self._raster_range(traj), self._traj_grain_dev(),
                                          corner_grains, out)

    @staticmethod
    def orientation_volume(volume, theta_z):
        """Grain ids -> misorientation angles in degrees, float32 with the volume's shape: the reference's
        theta_z[ids] / pi * 180 (pv_3Dview.py:150-192).  theta_z: [n_grain + 1] radians with entry 0 for uncovered pixels
        (traj.theta_z).  The table is formed in float64 on the host and rounded once; one gather on the device."""
        table = np.asarray(theta_z.detach().cpu().numpy() if torch.is_tensor(theta_z) else theta_z, np.float64).ravel()
        table = torch.from_numpy((table / np.pi * 180).astype(np.float32)).to(volume.device)
        if volume.numel() and not 0 <= int(volume.min()) <= int(volume.max()) < table.numel():
            raise _lib.GGNNError(f"the volume holds ids outside theta_z's 0..{table.numel() - 1}")
        return table[volume.long()]

    # -- the layers' grain-ID images (plot_polygons, graph_datastruct.py:553-610) ------------------------------
    def _raster_range(self, traj):
        """(g0, g1) of polygons(traj=...)'s slice (which has checked `traj` already)."""
        if traj is None:
            return None
        off = self._polygon_offsets()
        return int(off[0][int(traj)]), int(off[0][int(traj) + 1])

    def grain_image(self, size, layer=None, traj=None, corner_grains=None, out=None):
        """The grain-ID image of one recorded layer, filled on the device from its polygons: what the reference's
        traj.plot_polygons(size) leaves in `alpha_field` -- int32 [size[1], size[0]] (periodic: [size[0], size[0]]), indexed
        [y, x], pixel = the highest grain index + 1 among the polygons that hold it (include/ggnn.h,
        ggnn_polygons_rasterize: exact in integers), 0 = uncovered.  `layer` and `traj` as in polygons() (one
        synchronisation, the same errors; traj=t: ids local to the trajectory).  A no-flux image skips the boundary
        grain(s); corner_grains = (a, b, c, d) fills its uncovered pixels by quadrant.  On demand, on the current stream: the
        step, its graphs and the carried state are not touched."""
        k = self.polygons(layer, traj)["layer"]
        img = self.be.rasterize_polygons(self._poly["arena"], size, [k], self.boundary, self._raster_range(traj),
                                         self._traj_grain_dev(), corner_grains, None if out is None else out.unsqueeze(0))
        return img[0] if out is None else out

    def grain_images(self, size, layers=None, traj=None, corner_grains=None, out=None):
        """grain_image of several layers from one launch: int32 [L, ny, nx] -- the reference's `alpha_field_list`.
        layers: None = every layer recorded so far (of `traj`, where it ended early), or the layers to draw."""
        recorded = int(np.max(self.polygons(None, traj)["layers"]))
        if layers is None:
            layers = range(recorded + 1)
        layers = [int(k) for k in layers]
        cap = self._poly["capacity"]
        for k in layers:
            if not 0 <= k <= cap:
                raise _lib.GGNNError(f"layer {k} is outside the arena's 0..{cap}")
            if k > recorded:
                raise _lib.GGNNError(f"layer {k} has not been recorded: {recorded} layers so far")
        return self.be.rasterize_polygons(self._poly["arena"], size, layers, self.boundary, self._raster_range(traj),
                                          self._traj_grain_dev(), corner_grains, out)

    def image_error(self, image, truth=None):
        """An image against the phase-field map of its layer (compute_error_layer, graph_datastruct.py:346-348) and the
        pixel count of every id (the initial areas, :287), one launch: {'rate': differing / pixels, 'differing': int,
        'counts': int64 [n_grain + 1] on the device}; truth=None: the counts alone.  Integer atomics: exact."""
        if self._poly is None:
            raise _lib.GGNNError("call enable_polygons(...) first")
        if truth is not None:
            truth = torch.as_tensor(truth).to(device=image.device, dtype=torch.int32).contiguous()
        differing, counts = self.be.image_compare(image, truth, self.n_nodes["grain"])
        if truth is None:
            return {"counts": counts}
        differing = int(differing)
        return {"rate": differing / image.numel(), "differing": differing, "counts": counts}

    # -- what a step advances beside x: the QoI accumulator, the schedule's and the polygon recorder's counters -------------
    def _carried(self):
        """The device state a step advances beside x, each a dict with `home` (the rollout's own, advanced in place), `ring`
        / `entries` / `launched` / `at` (run_events' copies, _carry_enter_block) and `new` (makes one state; a state is copied
        through its `flat` tensor): the QoI accumulator (enable_qoi), the schedule's counter word (set_process_schedule) and
        the polygon recorder's layer word (enable_polygons)."""
        return [c for c in (self._qoi, self._sched, self._poly) if c is not None]

    @staticmethod
    def _carry_home_one(c):
        if c["at"] is not None:
            c["home"]["flat"].copy_(c["ring"][c["at"]]["flat"])
            c["at"] = None

    def _carry_home(self):
        """Behind run_events the current states are the last committed step's ring slot: back into the rollout's own."""
        for c in self._carried():
            self._carry_home_one(c)

    def _carry_take(self, pick):
        """The rollout's own states := `pick(c)` of every carried state c."""
        for c in self._carried():
            c["home"]["flat"].copy_(pick(c)["flat"])
            c["at"] = None

    def _carry_enter_block(self, slots):
        """Before a block of speculative steps: the slot before its first one holds the current states, and a copy of
        them is kept for the case that the block's first step is eventful (two full blocks in flight fill the ring: the last
        step of the second one overwrites that slot).  Two copies alternate: at most two blocks are unchecked.  Returns the
        copies by the states' names."""
        D, entries = self._spec["D"], {}
        for c in self._carried():
            if c["ring"] is None or len(c["ring"]) != D:
                self._carry_home_one(c)
                c["ring"], c["entries"] = [c["new"]() for _ in range(D)], [c["new"]() for _ in range(2)]
                self._invalidate_graphs(blocks=True)   # (the blocks' launches advance the ring's states)
            before = c["ring"][(slots[0] - 1) % D]
            if c["at"] != (slots[0] - 1) % D:
                self._carry_home_one(c)
                before["flat"].copy_(c["home"]["flat"])
            entry = entries[c["name"]] = c["entries"][c["launched"] & 1]
            c["launched"] += 1
            entry["flat"].copy_(before["flat"])
            c["at"] = slots[-1]
        return entries

    def qoi(self):
        """The quantities of interest up to the last step (one synchronisation).  For one trajectory: `volume` and `size`
        [n_grain] (device tensors: V0 + T + e of the last layer and cbrt(6 volume / pi) * mesh_size), `d_mu`, `d_std`
        (floats, over all grains, eliminated ones included, population std), `hist` (np.histogram(size, np.arange(0, 20,
        1 if n_grain > 400 else 2), density=True)), `hist_counts`, `bin_centres`, `layers` (steps accumulated) and, with a
        history, `volume_traj` [layers + 1, n_grain].  With traj_offsets: `d_mu` / `d_std` arrays and `hist` / `hist_counts` /
        `bin_centres` lists, one entry per trajectory.  With enable_events(traj_offsets=...): `layers` is an array, one
        entry per trajectory, and a trajectory that ended (trajectory_states) reports the volumes, sizes and layers of its
        last completed step; `volume_traj` keeps the union's rows.  Raises when a layer went beyond the history's capacity."""
        Q = self._qoi
        if Q is None:
            raise _lib.GGNNError("call enable_qoi(...) first")
        self._carry_home()
        H = Q["home"]
        T, e, ended = H["T"], H["e"], []
        if self._ens is not None:
            # a trajectory that ended keeps the accumulator rows and the layer count of its last completed step: patched into
            # a copy (one block per trajectory, position-independent: the finalize launch below sees nothing else of it)
            ens = self._ens["sessions"]
            ended = [(t, sn["qoi"]) for t, sn in enumerate(self._ens["snapshot"]) if sn is not None and sn["qoi"] is not None]
            if ended:
                T, e = T.clone(), e.clone()
                for t, q in ended:
                    g0, g1 = int(ens.grain_off[t]), int(ens.grain_off[t + 1])
                    T[g0:g1], e[g0:g1] = q["T"], q["e"]
        words = torch.cat([H["layer"], Q["words"][1:]] + [q["layer"] for _, q in ended]).cpu()
        layers = int(words[0])
        if int(words[1]) & _lib.GGNN_FLAG_QOI_OVERFLOW:
            raise _lib.GGNNError(f"the volume history has room for {Q['capacity']} layers, {layers} were accumulated: "
                                 "enable_qoi(capacity=...) or history=False")
        off, dev = Q["offsets_host"], self.x["grain"].device
        steps = [1 if n > 400 else 2 for n in np.diff(off)]   # graph_trajectory.py:251
        out, hist, counts, centres = None, [None] * len(steps), [None] * len(steps), [None] * len(steps)
        for step in sorted(set(steps)):
            edges = np.arange(0, 20, step).astype(np.float32)
            out = self.be.qoi_finalize(Q["V0"], T, e, Q["offsets"], Q["mesh_size"], torch.from_numpy(edges).to(dev))
            c = out[4].cpu().numpy().astype(np.int64)
            for t, st in enumerate(steps):
                if st == step:
                    counts[t] = c[t]
                    hist[t] = c[t] / max(int(c[t].sum()), 1) / np.diff(edges.astype(np.float64))
                    centres[t] = 0.5 * (edges[:-1] + edges[1:]).astype(np.float64)
        d_mu, d_std = out[2].cpu().numpy().astype(np.float64), out[3].cpu().numpy().astype(np.float64)
        one = len(steps) == 1
        res = {"volume": out[0], "size": out[1], "d_mu": float(d_mu[0]) if one else d_mu,
               "d_std": float(d_std[0]) if one else d_std, "hist": hist[0] if one else hist,
               "hist_counts": counts[0] if one else counts, "bin_centres": centres[0] if one else centres, "layers": layers}
        if Q["history"] is not None:
            res["volume_traj"] = Q["history"][:layers + 1]
        if self._ens is not None:   # per trajectory of the event layer: an ended one stopped counting
            per = np.full(self._ens["n_traj"], layers, dtype=np.int64)
            for k, (t, _) in enumerate(ended):
                per[t] = int(words[2 + k])
            res["layers"] = per
        return res

    # -- one step, enqueued on the current stream --------------------------------------
    def _pipelined(self):
        """Two streams and no joint launches: step() and run() enqueue the overlapped step (_enqueue_overlapped_step).
        Otherwise -- joint launches, one stream, or `_side = None` -- a step is _enqueue_forward_update + _enqueue_refresh."""
        return self._side is not None and not self.joint_launches

    def _enqueue_step(self):
        self._enqueue_steps(1)

    def _enqueue_steps(self, n_steps: int):
        if self._pipelined():
            return self._enqueue_steps_overlapped(n_steps)
        for _ in range(n_steps):
            self._enqueue_forward_update()
            self._enqueue_refresh()
        self._einfo_fresh = False
        self._x_written_outside()

    def _overlap_buffers(self):
        """The classifier's two alternating copies of x, indexed like the edge sets (outside any capture: _capture calls
        this first)."""
        if self._pipelined() and self._xcs is None:
            self._xcs = [{nt: torch.empty_like(self.x[nt]) for nt in NODE_TYPES} for _ in range(2)]
            self._xc_fresh = False

    def _heads_classifier(self, h_joint, ea, p):
        """The classifier's heads on the junction edges: `h_joint` and the lengths `ea` in, edge_event and edge of `p` out."""
        self.be.heads_classifier(h_joint, self.graph.edge_index[ET_JJ], ea[ET_JJ], self.w_cls[0], self.w_cls[1], self._tmp,
                                 p["edge_event"], p["edge"], E_dev=self.graph.csr[ET_JJ].E_dev)

    def _enqueue_overlapped_step(self, par, xc, xc_next, p, zf, headed_prev, slot=None):
        """One static-topology step on two streams with the regressor's tail -- heads + Rmodel.update, boundary step, grain
        centres, z clamp + edge lengths + the NEXT step's edge records -- UNDER the classifier's forward, where the chip
        would otherwise run the last workgroups of one decoder cell alone (profiles/r6_step_timeline.txt).  The regressor's
        chain stays on the current stream: it carries every step-to-step dependency.  The classifier reads its own copy of x
        (`xc`), and the copies of x, the edge lengths and the edge records alternate between two sets: this step reads
        `xc` and the lengths and records of set `par`, its refresh writes `xc_next` (ggnn_step_refresh_prepare's mirror, a
        by-product of its pass over the nodes) and the lengths and records of the other set, so nothing the tail writes is
        read by the classifier's forward of the same step.  Cross-stream edges:
          * the classifier waits for `ready`, recorded at the top of the step (its copy of x, the edge lengths and records
            are final);
          * the refresh, the first launch that writes into the set the previous step's classifier read, waits for that
            step's `headed_prev` (its heads, the last reader, are done).
        `p`: the predictions the heads write; `zf`: the z-clamp flag word Rmodel.update writes and the refresh reads.
        With a ring `slot` of the speculative event loop (_spec_state), the fused cells report to the slot's own range word,
        `updated` is recorded behind Rmodel.update, and the grain centres (noflux: and the junctions) as the step's events
        must see them -- before the boundary step and the centre refresh -- go to the slot's snapshots.
        Same kernels on the same operands as the single-stream plan: bit-identical results
        (test_pipelined_two_stream_rollout_equals_the_single_stream_plan).  Returns (ready, updated or None, headed): the
        caller keeps them alive until the streams are joined and a capture has ended."""
        be, x, S = self.be, self.x, self._spec
        ea, ea_next, einfo, einfo_next = self._ea[par], self._ea[1 - par], self._recs[par], self._recs[1 - par]
        main, st_c = torch.cuda.current_stream(), self._side[1]
        ready, headed = torch.cuda.Event(), torch.cuda.Event()
        updated = None if slot is None else torch.cuda.Event()
        word = self._range_word if slot is None else S["rw"][slot]   # (a void step's report is dropped with its slot)
        for name in ("R", "C"):
            self.ws[name].range_flag = word
        try:
            ready.record(main)
            enc, dec = self.packed["R"]
            hr, _ = run_encoder_decoder(be, enc, dec, self.graph, self.ws["R"], x, ea, einfo)
            with torch.cuda.stream(st_c):
                st_c.wait_event(ready)
                enc, dec = self.packed["C"]
                h, _ = run_encoder_decoder(be, enc, dec, self.graph, self.ws["C"], xc, ea, einfo)
                self._heads_classifier(h["joint"], ea, p)
                headed.record(st_c)
        finally:
            for name in ("R", "C"):
                self.ws[name].range_flag = self._range_word
        # heads + Rmodel.update in one launch; z clamp + edge lengths + next records + next copy of x in one launch
        be.heads_regressor_update(hr["joint"], hr["grain"], x["joint"], x["grain"], self.w_reg[0], self.w_reg[1],
                                  p["joint"], p["grain"], p["grain_area"], self.dz, self.zmax, zf)
        joints_before = centres_before = None
        if slot is not None:
            updated.record(main)
            joints_before, centres_before = (S["jb"][slot] if self.noflux else None), S["cen"][slot]
            if not self.refresh_centres:   # (otherwise the snapshot rides with the launch that replaces the centres)
                centres_before.copy_(x["grain"][:, :2])
        self._enqueue_tail(slot, joints_before, centres_before)
        if headed_prev is not None:
            main.wait_event(headed_prev)   # the previous step's classifier has read the set this refresh writes
        be.step_refresh_prepare(x["joint"], x["grain"], self.zmax, zf,
                                [(self.graph.csr[et], ea_next[et], x[et[0]], x[et[-1]], einfo_next[et])
                                 for et in EDGE_TYPES], mirror=(xc_next["joint"], xc_next["grain"]))
        return ready, updated, headed

    def _enqueue_steps_overlapped(self, n_steps: int):
        """`n_steps` overlapped steps (_enqueue_overlapped_step) on the rollout's own buffers, the other set current behind
        every step, no join between the steps; the classifier's stream is joined behind the last one.  Needs self.einfo to
        hold the records of the first step and the current copy of x to mirror x (step() / run() see to that:
        _ensure_edge_records)."""
        self._overlap_buffers()
        keep, headed = [], None
        for _ in range(n_steps):
            par = self._parity
            keep.append(self._enqueue_overlapped_step(par, self._xcs[par], self._xcs[1 - par], self.pred, self.flags, headed))
            headed = keep[-1][-1]
            self._parity = 1 - par
        torch.cuda.current_stream().wait_stream(self._side[1])
        self._next_step_prepared()
        return keep

    def _next_step_prepared(self):
        """Behind overlapped steps: the last refresh prepared the edge records of the step to come and left its mirror of x
        in the current copy (run_events' copies of x do not follow)."""
        self._einfo_fresh = self._xc_fresh = True
        if self._spec is not None:
            self._spec["xs_valid"] = None

    def _ensure_edge_records(self, mirror=True):
        """Before an overlapped step outside a capture: einfo must hold the records of the step to come and (`mirror`) the
        classifier's copy of x must equal x.  They are stale after construction, a topology change, an event-mode or
        single-stream step, and when the caller wrote into x / edge_attr (in-place Python writes bump the tensors' version
        counters; the kernels do not)."""
        seen = self._versions()
        if seen != self._seen:
            self._x_written_outside()
        if not self._einfo_fresh or seen != self._seen:
            prepare_edges(self.be, self.graph, self.x, self.edge_attr, self.einfo)
            self._einfo_fresh = True
        self._seen = seen
        if mirror and not self._xc_fresh:
            self._overlap_buffers()
            for nt in NODE_TYPES:
                self._xcs[self._parity][nt].copy_(self.x[nt])
            self._xc_fresh = True

    def _versions(self):
        """The version counters a caller's in-place write shows in: those of x and the one the views of the edge sets
        share -- a write into either set of lengths (or into anything else in the allocation) counts.  The rollout's own
        Python-side writes into the allocation bump it too: construction, which reads the counters anew (_cut_edge_sets),
        and _move_lengths_over, which takes its own write out again."""
        return tuple(t._version for t in self.x.values()) + (self._sets.buf._version,)

    def _move_lengths_over(self, parity: int):
        """Set `parity` becomes the current one with the lengths of the one that was (run_events' graphs alternate the sets
        by slot parity; step() / step_events() in between may have left the other set current).  The records and the
        classifier's copy of x do not follow."""
        unwritten = self._seen == self._versions()
        for et in EDGE_TYPES:
            self._ea[parity][et].copy_(self.edge_attr[et])
        if unwritten:   # (the copies bumped the allocation's counter; a caller's write from before still shows)
            self._seen = self._versions()
        self._parity = parity
        self._einfo_fresh = self._xc_fresh = False

    def _enqueue_forward_update(self, joint=None):
        """test.py:382-402: both forwards, Rmodel.update, z advance.  `joint`: True = the regressor and the classifier in the
        same launches whatever the rollout's plan (same kernels on the same operands, bit-identical results)."""
        be, x, ea, p = self.be, self.x, self.edge_attr, self.pred
        joint = self.joint_launches if joint is None else joint
        # edge geometry once per step, shared by both models and all four cells
        einfo = prepare_edges(be, self.graph, x, ea, self.einfo)

        def regressor():
            enc, dec = self.packed["R"]
            h, _ = run_encoder_decoder(be, enc, dec, self.graph, self.ws["R"], x, ea, einfo)
            be.heads_regressor(h["joint"], h["grain"], x["grain"], self.w_reg[0], self.w_reg[1],
                               p["joint"], p["grain"], p["grain_area"])

        def classifier(x_read=None):
            enc, dec = self.packed["C"]
            h, _ = run_encoder_decoder(be, enc, dec, self.graph, self.ws["C"], x, ea, einfo, x_read)
            self._heads_classifier(h["joint"], ea, p)

        if joint:
            run_encoder_decoder_multi(be, [(*self.packed["R"], self.ws["R"]), (*self.packed["C"], self.ws["C"])],
                                      self.graph, x, einfo)
            be.heads_regressor(self.ws["R"].h2["joint"], self.ws["R"].h2["grain"], x["grain"], self.w_reg[0],
                               self.w_reg[1], p["joint"], p["grain"], p["grain_area"])
            self._heads_classifier(self.ws["C"].h2["joint"], ea, p)
        elif self._side is None:
            regressor()
            classifier()
        else:
            # Two streams.  Rmodel.update (and the grain centres) need the regressor's heads only, and they may
            # overwrite x as soon as the classifier's last reader of x -- its decoder projection -- has run:
            # they go on the regressor's stream behind that event and hide beside the classifier's sweep, gate
            # GEMM and heads (the chip is otherwise nearly idle during these small launches).
            main = torch.cuda.current_stream()
            st_r, st_c = self._side
            x_free = torch.cuda.Event()
            st_r.wait_stream(main)
            st_c.wait_stream(main)
            with torch.cuda.stream(st_r):
                regressor()
            with torch.cuda.stream(st_c):
                classifier(lambda: x_free.record(st_c))
            with torch.cuda.stream(st_r):
                st_r.wait_event(x_free)
                be.step_update(x["joint"], x["grain"], p["joint"], p["grain"], self.dz, self.zmax, self.flags)
            main.wait_stream(st_r)
            main.wait_stream(st_c)
            return
        be.step_update(x["joint"], x["grain"], p["joint"], p["grain"], self.dz, self.zmax, self.flags)

    def _enqueue_tail(self, slot=None, joints_before=None, centres_before=None):
        """What follows Rmodel.update in every plan, in front of the launch that refreshes the edge lengths: boundary step
        (noflux), grain centres (refresh_centres), this step's QoI layer and its layer of polygons, the schedule's row of the
        step to come.  `slot`,
        `joints_before`, `centres_before`: the speculative event loop's (_enqueue_overlapped_step)."""
        self._enqueue_boundary(joints_before)
        if self.refresh_centres:
            self._enqueue_centres(centres_before)
        self._enqueue_qoi(slot)
        self._enqueue_polygons(slot)
        self._enqueue_schedule(slot)

    def _refresh_edges(self, lists, count_dev=None):
        """The edge list of a ggnn_step_refresh launch: the current lengths recomputed from x for `lists` ({edge type:
        edge_index}); `count_dev`: {edge type: the device word with the list's length at run time, or None}."""
        x, ea = self.x, self.edge_attr
        return [(lists[et], x[et[0]], x[et[-1]], ea[et]) + (() if count_dev is None else (count_dev[et],)) for et in EDGE_TYPES]

    def _enqueue_refresh(self):
        """test.py:405-407, [446-463 noflux], 468-478 + 556-559, 562-575: z clamp, boundary step, grain centres, edge
        lengths (of the full lists)."""
        self._enqueue_tail()
        self.be.step_refresh(self.x["joint"], self.x["grain"], self.zmax, self.flags,
                             self._refresh_edges(self.graph.edge_index, self.graph.count_dev))

    @staticmethod
    def _captured(enqueue):
        """A hipGraph (torch.cuda.CUDAGraph is hipGraph on ROCm) of the launches `enqueue()` makes through the C ABI,
        captured on a side stream: the capture records, it does not execute.  What `enqueue` returns (its stream events)
        lives until the capture has ended."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                keep = enqueue()
        torch.cuda.current_stream().wait_stream(s)
        del keep
        return g

    def _capture(self, n_steps: int = 1):
        """Record `n_steps` steps into a hipGraph, leaving the rollout's buffers as they were.  An overlapped step leaves
        the other set of edge lengths / edge records / copies of x current: a graph is only valid from the set it was
        captured on, so graphs are kept per parity (_replay), and an odd number of steps flips it after every replay."""
        self._overlap_buffers()
        state = (self._parity, self._einfo_fresh, self._xc_fresh)
        g = self._captured(lambda: self._enqueue_steps(n_steps))
        self._parity, self._einfo_fresh, self._xc_fresh = state
        return g

    def _replay(self, n_steps: int):
        """`n_steps` steps from the hipGraph captured for this step count and the current set of buffers."""
        if self._graphs is None:
            self._graphs = {}
        key = (n_steps, self._parity)
        g = self._graphs.get(key)
        if g is None:
            g = self._graphs[key] = self._capture(n_steps)
        g.replay()
        if self._pipelined():
            self._parity ^= n_steps & 1
            self._next_step_prepared()
        else:
            self._einfo_fresh = False
            self._x_written_outside()

    # -- event-driven mode ------------------------------------------------
    def enable_events(self, mask, area_threshold: float = 1e-4, edge_threshold: float = 0.6, traj_offsets=None):
        """Switch to the full loop of test.py:382-575: after the device forwards + Rmodel.update,
        grains whose predicted area fell below `area_threshold` (Rmodel.threshold, test.py:187,
        418) are eliminated and junction edges with sigmoid(edge_event) above `edge_threshold`
        (Cmodel.threshold, :188) are switched by the host-side `topology.update_topology`; then
        grain centres and edge lengths are refreshed on the NEW topology.  `mask` = the
        reference's `data['mask']` ({'grain': [N_g, 1], 'joint': [N_j, 1]}, any integer dtype).
        traj_offsets: None, or {'grain': [n_traj + 1], 'joint': [n_traj + 1]} -- the graph is a disjoint union of
        trajectories (node offsets rising from 0 to the node counts, as in enable_qoi) and the events are detected, applied
        and refused PER TRAJECTORY: a trajectory whose update is refused ends, the others go on
        (trajectory_states).  A no-flux union (constructor traj_offsets) uses the constructor's offsets: None here, or equal
        ones; every trajectory's boundary grain stays out of its candidates."""
        if self.noflux:   # (a no-flux union has the constructor's offsets and no others)
            own = resolve_traj_offsets(None if self._traj is None else (self._traj["grain"], self._traj["joint"]), traj_offsets,
                                       "enable_events")
            traj_offsets = None if own is None else {"grain": own[0], "joint": own[1]}
        ens = None if traj_offsets is None else self._ensemble_sessions(traj_offsets)
        self.mask = {k: np.array(torch.as_tensor(mask[k]).cpu().numpy(), dtype=np.int64, copy=True).reshape(-1, 1)
                     for k in ("grain", "joint")}
        dev = self.x["joint"].device
        self._live_grain = torch.from_numpy(self.mask["grain"][:, 0].astype(np.int32)).to(dev)
        # what the device-side count reads as its live mask.  A no-flux union: a second mask with every boundary grain's word
        # at 0 (ggnn_detect_events_traj takes no grain to skip; the live mask itself keeps 1 there: the QoI reads it)
        self._cand_grain = self._live_grain
        if self._traj is not None:
            self._cand_grain = torch.from_numpy(self._candidate_mask()).to(dev)
        self.area_threshold, self.edge_threshold = float(area_threshold), float(edge_threshold)
        # device-side trigger: slightly wider than the host's exact sigmoid(x) > threshold test,
        # so a borderline edge always reaches the host, which then decides exactly
        self._logit_trigger = float(np.log(edge_threshold / (1.0 - edge_threshold)) - 1e-4)
        self._ev_flags = torch.zeros(2, dtype=torch.int32, device=dev)
        self._ev_host = torch.zeros(2, dtype=torch.int32).pin_memory()
        self._quiet_steps = 0
        # (a new live mask, which the QoI launches read from now on; the blocks go with the edge sets: _enter_capacity_mode)
        self._invalidate_graphs(static=self._qoi is not None, segments=True)
        self.grain_events, self.switched = [], []
        self._enter_capacity_mode()
        self._ens = None
        if ens is not None:
            self._enable_ensemble(ens)

    # -- events per trajectory of a disjoint union --------------------------------------------------------------
    def _ensemble_sessions(self, traj_offsets):
        """One topology session per trajectory from the current lists (one read-back); GGNNError unless they are a disjoint
        union with the segments in trajectory order."""
        from .topology import EnsembleSessions, check_traj_offsets, union_edge_segments
        og, oj = check_traj_offsets(traj_offsets, self.n_nodes["grain"], self.n_nodes["joint"])
        union_edge_segments(self.edge_index[GJ].cpu().numpy(), og, oj, "grain-junction list")
        return EnsembleSessions(self.edge_index[ET_JJ].cpu().numpy(), self.edge_index[JG].cpu().numpy(), og, oj)

    def _candidate_mask(self, out=None):
        """The live mask with the boundary grains' words at 0 (int32 [n_grain]; `out`: a pinned staging array)."""
        cand = self.mask["grain"][:, 0].astype(np.int32) if out is None else out
        if out is not None:
            out[:] = self.mask["grain"][:, 0]
        cand[self._traj["boundary_grains"]] = 0
        return cand

    def _host_masks(self):
        """The host masks (grain, joint) as the sessions patch them in place: contiguous int64 (a caller may have replaced
        them by something else)."""
        mg, mj = self.mask["grain"], self.mask["joint"]
        if not (mg.dtype == np.int64 and mg.flags.c_contiguous and mj.dtype == np.int64 and mj.flags.c_contiguous):
            mg, mj = self.mask["grain"], self.mask["joint"] = np.ascontiguousarray(mg, np.int64), np.ascontiguousarray(mj, np.int64)
        return mg, mj

    def _enable_ensemble(self, ens):
        """The device side of the per-trajectory layer: the offsets, the `ended` words and ONE buffer of 2 + 2 n_traj count
        words (totals first: step_events reads them as it reads the two words of a single trajectory)."""
        dev, n = self.x["joint"].device, ens.n_traj
        self._ev_flags = torch.zeros(2 + 2 * n, dtype=torch.int32, device=dev)
        self._ev_host = torch.zeros(2 + 2 * n, dtype=torch.int32).pin_memory()
        self._ens = {
            "sessions": ens, "n_traj": n, "grain_off": torch.from_numpy(ens.grain_off).to(dev),
            "joint_off": torch.from_numpy(ens.joint_off).to(dev), "ended": torch.zeros(n, dtype=torch.int32, device=dev),
            "ended_host": torch.zeros(n, dtype=torch.int32).pin_memory(), "ended_at": [None] * n, "error": [None] * n,
            "snapshot": [None] * n, "rewired": 0}

    def _rewire_union(self):
        """_rewire for a union: every trajectory with candidates gets its own update from its own session
        (topology.EnsembleSessions.apply); a refused one ends (_end_trajectory).  Same return value."""
        E, N = self._ens, self._evb["np"]
        ens, n_e = E["sessions"], self.edge_index[ET_JJ].size(1)
        if ens.n_pp != n_e:
            raise _lib.GGNNError("the topology sessions and the rollout's junction edge list disagree")
        mg, mj = self._host_masks()
        E["rewired"] += 1
        ended = E["ended_host"].numpy()
        res = ens.apply(N["xj"], N["yj"], N["yg"][:, 0], N["prob"][:n_e], N["area"], mg, mj, self._ev_host.numpy()[2:], ended,
                        self.area_threshold, self.edge_threshold, N["lists"], skip_local_grain=0 if self.noflux else None)
        for t, message in res["refused"].items():
            self._end_trajectory(t, message)
        if res["refused"]:
            E["ended"].copy_(E["ended_host"], non_blocking=True)
        if not res["changed"]:
            return None
        return res["events"], res["switches"], res["n_pp"], res["n_pq"]

    def _end_trajectory(self, t, message):
        """Trajectory t's update was refused: it takes part in no events from now on, and what its own rollout would hold
        where its step_events() raised -- features updated, topology and masks untouched, the accumulator of the layers
        completed so far -- is kept (device-side copies, ordered before anything that overwrites the rows)."""
        E = self._ens
        ens = E["sessions"]
        g0, g1, j0, j1 = (int(v) for v in (ens.grain_off[t], ens.grain_off[t + 1], ens.joint_off[t], ens.joint_off[t + 1]))
        snap = {"x_joint": self.x["joint"][j0:j1].clone(), "x_grain": self.x["grain"][g0:g1].clone(),
                "mask": {"grain": self.mask["grain"][g0:g1].copy(), "joint": self.mask["joint"][j0:j1].copy()},
                "edge_index": ens.local_lists(t), "steps": self.steps_done, "qoi": None,
                "poly_layer": None if self._poly is None else self._poly["home"]["layer"].clone()}
        if self._qoi is not None:
            H = self._qoi["home"]
            snap["qoi"] = {"T": H["T"][g0:g1].clone(), "e": H["e"][g0:g1].clone(), "a": H["a"][g0:g1].clone(),
                           "layer": H["layer"].clone()}
        E["snapshot"][t], E["ended_at"][t], E["error"][t] = snap, self.steps_done, message
        E["ended_host"][t] = 1

    def trajectory_states(self):
        """Per trajectory of enable_events(traj_offsets=...): a list of dicts with `x_joint`, `x_grain` (device tensors),
        `mask` ({'grain', 'joint'}: int64 [n, 1]), `edge_index` (the three lists in the trajectory's own indices, numpy),
        `ended_at` (the number of steps it completed when its update was refused; None while it runs) and `error` (the
        refusal's message).  A running trajectory: views of its live rows; an ended one: what its own rollout held when its
        step_events() raised."""
        E = self._ens
        if E is None:
            raise _lib.GGNNError("call enable_events(mask, ..., traj_offsets=...) first")
        ens, out = E["sessions"], []
        for t in range(E["n_traj"]):
            snap = E["snapshot"][t]
            if snap is None:
                g0, g1, j0, j1 = (int(v) for v in (ens.grain_off[t], ens.grain_off[t + 1], ens.joint_off[t], ens.joint_off[t + 1]))
                snap = {"x_joint": self.x["joint"][j0:j1], "x_grain": self.x["grain"][g0:g1],
                        "mask": {"grain": self.mask["grain"][g0:g1].copy(), "joint": self.mask["joint"][j0:j1].copy()},
                        "edge_index": ens.local_lists(t)}
            out.append({"x_joint": snap["x_joint"], "x_grain": snap["x_grain"], "mask": snap["mask"],
                        "edge_index": snap["edge_index"], "ended_at": E["ended_at"][t], "error": E["error"][t]})
        return out

    def _skip_grain(self):
        """The grain that never takes part in events: the no-flux boundary grain (test.py:421-422), or none."""
        return 0 if self.noflux else -1

    def _run_segment(self, which):
        """The two halves of a step, replayed from their own hipGraphs: on the in-place topology (_enter_capacity_mode) from the
        first step on and across events; otherwise once the topology has been quiet for two steps (an event then drops the
        graphs with the topology, and a capture is not worth it while events fire every step)."""
        fn = self._enqueue_forward_update if which == "fwd" else self._enqueue_refresh
        in_place = self._cap is not None   # (the graphs survive events: captured once, at the first step)
        if self.use_graph and (self._quiet_steps >= 2 or in_place):
            # a segment graph holds the addresses of the buffers it reads and writes; run_events() leaves other ones current
            # (its slots' predictions, the other set of edge lengths / records): a graph per set.  The forwards read the edge
            # lengths and records and write the predictions; the refresh writes the edge lengths.  (Everything else a
            # segment holds is dropped with what replaces it: _invalidate_graphs)
            key = (which, self._parity, self._pred_at) if which == "fwd" else (which, self._parity)
            g = self._segment_graphs.get(key)
            if g is None:
                if in_place:   # valid for as long as no list is longer than now (_install_topology_in_place)
                    self._cap["captured"] = self._smallest_sizes(self._cap["captured"])
                g = self._segment_graphs[key] = self._captured(fn)
            if which == "fwd":
                self._graph_fwd = g
            else:
                self._graph_ref = g
            g.replay()
        elif which == "fwd":
            # eager launches (GGNN_EVENT_GRAPHS=0 / a caller's own topology: the steps around an event, which replaces the
            # topology the graphs were captured on) are bound by the HOST's launch rate at any graph size -- ~20 launches +
            # stream forks of the two-stream plan take 0.49 ms where the kernels take 0.35
            # (profiles/r6_event_step_breakdown.txt): R and C share every launch here
            self._enqueue_forward_update(joint=True)
        else:
            fn()

    def step_events(self):
        """One step with topological events.  Returns (pred, grain_events, switching_list); the
        last two are empty numpy arrays on a quiet step.  One 8-byte read-back per step is the only
        host synchronisation unless an event fires."""
        if self.mask is None:
            raise _lib.GGNNError("call enable_events(mask, ...) first")
        self.refresh_weights(sample=self.steps_done % 16 != 0)
        self._carry_home()
        self._einfo_fresh = False   # this mode prepares its edge records at the start of every step
        self._x_written_outside()
        self._run_segment("fwd")
        p = self.pred
        if self._ens is None:
            self.be.detect_events(p["grain_area"], self._live_grain, self.area_threshold, p["edge_event"],
                                  self.graph.edge_index[ET_JJ], self._logit_trigger, self._ev_flags, skip_grain=self._skip_grain())
        else:   # per trajectory: [2 + 2 n_traj] words, the totals over the running trajectories first
            E = self._ens
            self.be.detect_events_traj(p["grain_area"], self._cand_grain, self.area_threshold, p["edge_event"],
                                       self.graph.edge_index[ET_JJ], self._logit_trigger, E["grain_off"], E["joint_off"],
                                       self._ev_flags[2:], self._ev_flags[:2], ended=E["ended"])
        self._ev_host.copy_(self._ev_flags, non_blocking=True)
        # behind an eventful step the next one is eventful too, on the reference's trajectories (README.md:68-69: events at
        # nearly every step): what the rewiring reads travels to the host behind the counts, one synchronisation instead of two
        payload = self._quiet_steps == 0 and self._evb is not None
        if payload:
            self._enqueue_event_readback()
        torch.cuda.current_stream().synchronize()
        events, switches = np.zeros(0, np.int64), np.zeros((0, 2), np.int64)
        pred = self.pred
        if int(self._ev_host[0]) or int(self._ev_host[1]):
            # _apply_events may replace the topology and with it the per-edge output buffers:
            # the caller gets this step's predictions on the PRE-event edge list, as the
            # reference's loop does (test.py:383-426 keeps `pred` across Cmodel.update)
            pred = dict(self.pred)
            events, switches = self._apply_events(payload_ready=payload)
        if len(events) or len(switches):
            self._quiet_steps = 0
        else:
            self._quiet_steps += 1
        self._run_segment("ref")
        self.steps_done += 1
        self.grain_events.append(events)
        self.switched.append(switches)
        return pred, events, switches

    # -- event-driven mode without a host stall per quiet step ------------------------------------------------------
    # steps per block in run_events while the topology is quiet (a graph-to-graph boundary costs ~25 us at the 10k-grain
    # graph); after an eventful step the blocks start again at one step and double while the steps stay quiet (on the in-place
    # topology their graphs are the ones captured before the event; otherwise every event drops them with the topology)
    EVENTS_UNROLL = 8

    def _spec_state(self):
        """Buffers of the speculative event loop (run_events): a ring of 2 x EVENTS_UNROLL slots, slot = step index mod
        ring size -- x as the step found it (the copy the classifier's forward reads anyway: written by the refresh of
        the step before, ggnn_step_refresh_prepare's mirror), the step's predictions, the grain centres as they were
        before the step's refresh, its z-clamp flag (test.py:405: written by the step's Rmodel.update, read by its
        refresh), its event counts and its own fp16-range word (device + pinned host: [grains, edges, range, -]) --
        the step of a slot reads the set of edge lengths / edge records of the slot's parity, so the rollout's parity follows
        the current slot.  Graphs are captured per (first slot, number of steps).  On the in-place topology
        (_enter_capacity_mode) the ring and the graphs survive events (the views are re-cut); otherwise the per-edge half and
        the graphs are rebuilt after every topology change."""
        S, dev = self._spec, self.x["joint"].device
        D = 2 * max(1, int(self.EVENTS_UNROLL))
        if S is None or S["D"] != D:
            # the per-node slots, the centre snapshots and the (pinned) count words: the node sets never change
            per_edge = ("edge_event", "edge")   # the predictions that follow the junction edge list
            S = self._spec = {
                "cur": self._parity, "D": D, "graphs": {}, "captured": None, "xs_valid": None, "topology": None, "sets": None,
                "flat": None, **self._spec_node_slots(D),
                "pred": [{k: torch.empty_like(v) for k, v in self.pred.items() if k not in per_edge} for _ in range(D)]}
            # (a segment graph captured while self.pred was a slot of the ring before holds that slot's predictions)
            self._invalidate_graphs(segments=True)
        if S["topology"] is not self.graph or S["sets"] is not self._sets:
            # The slots' per-edge predictions are cut from one allocation of the edge sets' capacity.  While the topology
            # lives in place (_enter_capacity_mode) the edge sets are the SAME allocations before and after an event, and the
            # graphs of the blocks -- whose per-edge kernels read the number of edges from device memory -- stay valid
            # across events for as long as no list has grown: an event re-cuts the views, nothing else.  Otherwise an event
            # brings new edge sets (and has dropped the graphs with the old ones: _set_topology).
            Ea = (self._sets.capacity[ET_JJ] + 3) & ~3                        # (16-byte aligned segments)
            if S["sets"] is not self._sets:
                S["flat"] = torch.empty(3 * D * Ea, dtype=torch.float32, device=dev)   # one allocation for all slots
            for slot, edge in zip(S["pred"], self._spec_edge_slots(S["flat"], D, Ea)):
                slot.update(edge)
            S["in_place"], S["topology"], S["sets"] = self._cap is not None, self.graph, self._sets
            self._invalidate_graphs(blocks=self._outgrown(S["captured"]))
        if (S["cur"] & 1) != self._parity:   # (step() / step_events() in between left the other set current)
            self._move_lengths_over(S["cur"] & 1)
        return S

    def _spec_node_slots(self, D: int):
        """The per-node buffers of the ring's `D` slots (_spec_state)."""
        dev = self.x["joint"].device
        return {"xs": [{nt: torch.empty_like(self.x[nt]) for nt in NODE_TYPES} for _ in range(D)],
                "cen": [torch.empty(self.n_nodes["grain"], 2, device=dev) for _ in range(D)],
                "jb": [torch.empty(self.n_nodes["joint"], 2, device=dev) for _ in range(D)],
                "evf": [torch.zeros(4, dtype=torch.int32, device=dev) for _ in range(D)],
                "evh": [torch.zeros(4, dtype=torch.int32).pin_memory() for _ in range(D)],
                "zf": [torch.zeros(2, dtype=torch.int32, device=dev) for _ in range(D)],
                "rw": [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(D)]}

    def _spec_edge_slots(self, flat, D: int, Ea: int):
        """The per-edge predictions of the ring's `D` slots for the current junction edge list, cut from `flat` (3 x Ea
        floats per slot)."""
        E = self.pred["edge_event"].numel()
        return [{"edge_event": flat[3 * i * Ea:3 * i * Ea + E], "edge": flat[3 * i * Ea + Ea:3 * i * Ea + Ea + 2 * E].view(E, 2)}
                for i in range(D)]

    def _enqueue_spec_steps(self, slots):
        """The steps of a block with events ASSUMED ABSENT: the overlapped step (_enqueue_overlapped_step) on the edge set of
        the slot's parity and the slot's buffers -- nothing an event would need is overwritten by the steps enqueued behind
        it: they use other slots of the ring (the copy of x the step leaves for the next one, its z-clamp flag and its range
        word included) -- each followed by the event counts of its predictions (ggnn_detect_events) copied to pinned host
        memory.  The streams are joined behind the last step.  Needs S["xs"][slots[0]] to equal x (_spec_launch)."""
        S, be = self._spec, self.be
        main, st_d = torch.cuda.current_stream(), self._side[0]   # (the event counts on a stream of their own: neither
        keep, headed = [], None                                   #  model's chain waits for them)
        for slot in slots:
            p = S["pred"][slot]
            ready, updated, headed = self._enqueue_overlapped_step(
                slot & 1, S["xs"][slot], S["xs"][(slot + 1) % S["D"]], p, S["zf"][slot], headed, slot)
            keep.append((ready, updated, headed))
            with torch.cuda.stream(st_d):
                st_d.wait_event(updated)   # grain_area of this step (and every cell of the regressor has reported its range)
                st_d.wait_event(headed)    # ... and its edge_event (the classifier's cells have, too)
                # (the slot's range word travels in flags[2] and is cleared by the same launch: it is sticky on the device)
                be.detect_events(p["grain_area"], self._live_grain, self.area_threshold, p["edge_event"],
                                 self.graph.edge_index[ET_JJ], self._logit_trigger, S["evf"][slot], S["rw"][slot],
                                 E_dev=self.graph.csr[ET_JJ].E_dev, skip_grain=self._skip_grain())
                S["evh"][slot].copy_(S["evf"][slot], non_blocking=True)
        main.wait_stream(self._side[1])
        main.wait_stream(st_d)
        return keep

    def _spec_launch(self, n: int):
        """Enqueue `n` speculative steps from the current slot on; returns (their slots, the event behind them, the QoI
        accumulator and the schedule counter the block started from: _carry_enter_block)."""
        S = self._spec
        slots = [(S["cur"] + i) % S["D"] for i in range(n)]
        if S["xs_valid"] != slots[0]:   # the first step's copy of x (later ones get theirs from the refresh before them)
            for nt in NODE_TYPES:
                S["xs"][slots[0]][nt].copy_(self.x[nt])
        S["xs_valid"] = (slots[-1] + 1) % S["D"]
        self._xc_fresh = False
        entry = self._carry_enter_block(slots)
        if self.use_graph and n > 1:
            g = S["graphs"].get((slots[0], n))
            if g is None:
                if S["in_place"]:   # valid for as long as no list is longer than now (_spec_state)
                    S["captured"] = self._smallest_sizes(S["captured"])
                g = S["graphs"][(slots[0], n)] = self._captured(lambda: self._enqueue_spec_steps(slots))
            g.replay()
        else:
            self._enqueue_spec_steps(slots)
        done = torch.cuda.Event()
        done.record()
        self._spec_adopt(slots[-1])
        self._einfo_fresh = True   # (the last step's refresh prepared the records of the step to come)
        return slots, done, entry

    def _spec_adopt(self, slot: int):
        """The rollout's current buffers := the state behind the step of `slot`."""
        S = self._spec
        self.pred, self._pred_at = S["pred"][slot], 1 + slot
        self._parity = (slot + 1) & 1
        S["cur"] = (slot + 1) % S["D"]

    def run_events(self, n_steps: int):
        """`n_steps` steps of the full loop of test.py:382-575 (forwards, Rmodel.update, topological events, grain
        centres, edge refresh) WITHOUT a host stall per quiet step: the steps are enqueued EVENTS_UNROLL at a time as if
        they had no events (one captured graph per block), each step's event counts travel to pinned host memory, and
        the host reads the counts of a block only after the next block is enqueued -- the device never waits for the
        host while the topology is quiet.  When a step did have events, every step enqueued behind it is void: x is
        taken back from the copy the following step made at its top, the grain centres from the snapshot taken before
        the eventful step's refresh, that step's predictions are still in their own slot; the events are then applied
        exactly as step_events does (host-side topology update, refresh on the new topology) and the loop goes on from
        the next step.  Same results, bit for bit, as n_steps x step_events()
        (test_speculative_event_loop_equals_step_events).  Needs the two-stream launch plan (joint_launches=False,
        concurrent=True); otherwise runs step_events in a loop.  Returns (grain_events, switching_lists): one entry per step."""
        if self.mask is None:
            raise _lib.GGNNError("call enable_events(mask, ...) first")
        if self._ens is not None:
            raise _lib.GGNNError("run_events() does not run on a union with traj_offsets (nearly every union step is "
                                 "eventful: speculation buys nothing); call step_events()")
        if not self._pipelined():
            out = [self.step_events()[1:] for _ in range(n_steps)]
            return [e for e, _ in out], [sw for _, sw in out]
        self.refresh_weights()
        ev_out, sw_out = [], []
        none = (np.zeros(0, np.int64), np.zeros((0, 2), np.int64))

        def finish(step_events):   # book-keeping of one completed step
            ev_out.append(step_events[0])
            sw_out.append(step_events[1])
            self.grain_events.append(step_events[0])
            self.switched.append(step_events[1])
            self.steps_done += 1

        K = max(1, int(self.EVENTS_UNROLL))
        quiet_blocks = self._spec_quiet_blocks
        blocks = []   # enqueued, unchecked: (slots, done event), oldest first
        while len(ev_out) < n_steps:
            in_flight = sum(len(b[0]) for b in blocks)
            if len(blocks) < 2 and len(ev_out) + in_flight < n_steps:
                self._spec_state()
                self._ensure_edge_records(mirror=False)
                size = min(K, 1 << min(quiet_blocks + len(blocks), 16))
                size = min(size, K - self._spec["cur"] % K)   # blocks end on multiples of K: full blocks reuse two graphs
                blocks.append(self._spec_launch(min(size, n_steps - len(ev_out) - in_flight)))
                if len(blocks) < 2 and len(ev_out) + in_flight + len(blocks[-1][0]) < n_steps:
                    continue   # keep one block queued behind the one whose counts are read
            S = self._spec
            slots, done, entry = blocks.pop(0)
            done.synchronize()
            hit = next((i for i, sl in enumerate(slots) if int(S["evh"][sl][0]) or int(S["evh"][sl][1])), None)
            # the fp16-range reports of the steps that stand (a void step ran on a topology the trajectory never had)
            if any(int(S["evh"][sl][2]) for sl in (slots if hit is None else slots[:hit + 1])):
                self._range_hit = True
            if hit is None:
                for _ in slots:
                    finish(none)
                quiet_blocks += 1
                self._spec_quiet_blocks = quiet_blocks
                continue
            quiet_blocks = self._spec_quiet_blocks = 0
            for _ in range(hit):
                finish(none)
            slot = slots[hit]
            # the step of `slot` saw events: whatever was enqueued behind it is void
            torch.cuda.current_stream().synchronize()
            void = len(slots) - hit - 1 + sum(len(b[0]) for b in blocks)
            blocks = []
            self._x_written_outside()
            # the z-clamp flag as the eventful step's Rmodel.update left it (test.py:405): the refreshes below read it
            self.flags.copy_(S["zf"][slot])
            if void:
                nxt = S["xs"][(slot + 1) % S["D"]]
                for nt in NODE_TYPES:
                    self.x[nt].copy_(nxt[nt])                # x as the step behind found it (= after the eventful step)
                self._spec_adopt(slot)
                # the void steps refreshed the edge sets past this point: lengths and records are recomputed from x below
                self._einfo_fresh = False
            # the accumulator and the schedule's counter as the eventful step found them: its layer is computed, its row of
            # the step to come written again (the same row: the tail is idempotent there)
            self._carry_take(lambda c: c["ring"][slots[hit - 1]] if hit else entry[c["name"]])
            keep_centres = self.x["grain"][:, :2].clone()
            self.x["grain"][:, :2].copy_(S["cen"][slot])     # the centres the events must see: before the refresh
            if self.noflux:   # ... and the junctions: before the boundary step
                keep_joints = self.x["joint"][:, :2].clone()
                self.x["joint"][:, :2].copy_(S["jb"][slot])
            def stands():   # the step stands as enqueued (its refresh ran on the unchanged topology)
                self.x["grain"][:, :2].copy_(keep_centres)
                self._carry_take(lambda c: c["ring"][slot])
                if self.noflux:
                    self.x["joint"][:, :2].copy_(keep_joints)
                if void:   # ... but its edge lengths were overwritten by the void steps: the same kernel on the same x
                    self.be.step_refresh(self.x["joint"], self.x["grain"], self.zmax, self.flags,
                                         self._refresh_edges(self.graph.edge_index))
            try:
                events, switches = self._apply_events()
            except Exception:
                # the host-side update refused the events (it leaves masks, coordinates and edge lists untouched): the step
                # is kept as a quiet one, so that a caller who catches the error can go on from a consistent state
                stands()
                finish(none)
                raise
            if len(events) or len(switches):
                self._quiet_steps = 0
                self._run_segment("ref")                     # centres + edge lengths on the new topology
                self._einfo_fresh = False
            else:   # the device-side trigger was conservative
                stands()
            finish((events, switches))
        return ev_out, sw_out

    def _event_buffers(self):
        """Pinned host staging of the event round trip, sized once (the lists only shrink: a removed grain appends two
        junction columns and drops at least eight; a list that grows past its room gets new buffers)."""
        E, n_pq = self.edge_index[ET_JJ].size(1), self.edge_index[JG].size(1)
        B = self._evb
        if B is not None and B["cap"] >= 2 * (E + n_pq) and B["prob_cap"] >= E:
            return B
        nj, ng = self.n_nodes["joint"], self.n_nodes["grain"]
        fj = self.x["joint"].size(1)
        cap = 2 * (E + n_pq) + 1024
        f = torch.empty(ng + (E + 512) + nj * fj + 2 * nj + 2 * ng, dtype=torch.float32).pin_memory()
        o = [0]

        def take(n, shape):
            v = f[o[0]:o[0] + n].view(shape)
            o[0] += n
            return v
        B = self._evb = {"cap": cap, "prob_cap": E + 512, "area": take(ng, (ng,)), "prob": take(E + 512, (E + 512,)),
                         "xj": take(nj * fj, (nj, fj)), "yj": take(2 * nj, (nj, 2)), "yg": take(2 * ng, (ng, 2)),
                         "lists": torch.empty(cap, dtype=torch.int64).pin_memory(),
                         "live": torch.empty(ng, dtype=torch.int32).pin_memory()}
        B["np"] = {k: B[k].numpy() for k in ("area", "prob", "xj", "yj", "yg", "lists", "live")}
        if self._traj is not None:   # (the candidate mask of a no-flux union follows the live mask)
            B["cand"] = torch.empty(ng, dtype=torch.int32).pin_memory()
            B["np"]["cand"] = B["cand"].numpy()
        return B

    def _topology_session(self):
        """The library-side lists of this trajectory (topology.TopologySession): opened from the device lists at the first
        event (one read-back), afterwards patched by every update -- as long as the rollout's edge lists are the ones the
        session produced last."""
        from .topology import TopologySession
        jj, jg = self.edge_index[ET_JJ], self.edge_index[JG]
        T = self._topo
        if T is not None and T[1] is jj and T[2] is jg and T[3] == (jj._version, jg._version):
            return T[0]
        if T is not None:
            T[0].close()
        ses = TopologySession(jj.cpu().numpy(), jg.cpu().numpy(), self.n_nodes["joint"], self.n_nodes["grain"])
        self._topo = (ses, jj, jg, (jj._version, jg._version))
        return ses

    def _enqueue_event_readback(self):
        """What the rewiring reads -- predicted areas, switching probabilities, junction coordinates and displacements -- as
        asynchronous copies into the pinned staging buffers (the caller synchronises)."""
        B, p = self._event_buffers(), self.pred
        E = self.edge_index[ET_JJ].size(1)
        prob_d = torch.sigmoid(p["edge_event"])
        B["area"].copy_(p["grain_area"], non_blocking=True)
        B["prob"][:E].copy_(prob_d, non_blocking=True)
        B["xj"].copy_(self.x["joint"], non_blocking=True)
        B["yj"].copy_(p["joint"], non_blocking=True)
        B["yg"].copy_(p["grain"], non_blocking=True)

    def _apply_events(self, payload_ready=False):
        """Host round trip of an eventful step: the predictions and junction coordinates travel to pinned host memory in
        one batch of asynchronous copies behind ONE synchronisation (_read_back_events), the library's session rewires its
        lists in place (_rewire), the new lists, coordinates and masks travel back asynchronously (_upload_events) and the
        CSR tables are rebuilt without a read-back (_install_event_topology) -- the host returns to enqueueing the next step
        while the device is still uploading (profiles/r6_event_step_breakdown.txt).  Returns (grain events, switched edges)."""
        self._read_back_events(payload_ready)
        rewired = self._rewire(self._grain_candidates()) if self._ens is None else self._rewire_union()
        if rewired is None:
            return np.zeros(0, np.int64), np.zeros((0, 2), np.int64)
        events, switches, n_pp, n_pq = rewired
        self._install_event_topology(self._upload_events(events, n_pp, n_pq))
        return events, switches

    def _read_back_events(self, payload_ready=False):
        """What the rewiring reads, in the pinned staging buffers, and the host synchronised with the device
        (`payload_ready`: step_events enqueued the copies behind the step's event counts and has synchronised)."""
        if not payload_ready:
            self._enqueue_event_readback()
            torch.cuda.current_stream().synchronize()

    def _grain_candidates(self):
        """test.py:418-422: the live grains whose predicted area fell below the threshold, smallest first; for noflux never
        the boundary grain."""
        area = self._evb["np"]["area"]
        live = self.mask["grain"][:, 0] > 0
        ge = np.flatnonzero(live & (area < np.float32(self.area_threshold)))
        ge = ge[np.argsort(area[ge], kind="stable")]
        if self.noflux:
            ge = ge[ge != 0]
        return ge

    def _rewire(self, ge):
        """The library's session applies the step's events to its lists, the masks and the staged junction coordinates and
        displacements (ggnn_topology_apply: a refused update leaves everything as it was) and exports its new lists into
        the pinned list buffer.  Returns (grain events, switched edges, junction edges, junction-grain edges), or None when
        nothing changed: the session ignores edges at or below the threshold and the (dst, src) twin of every pair, so with
        no grain below the area threshold either the update is the identity (the device-side trigger was conservative)."""
        ses = self._topology_session()
        N = self._evb["np"]
        E = self.edge_index[ET_JJ].size(1)
        if ses.n_pp != E:
            raise _lib.GGNNError("the topology session and the rollout's junction edge list disagree")
        mg, mj = self._host_masks()
        events, switches = ses.apply(N["xj"], N["yj"], N["yg"][:, 0], N["prob"][:E], ge, mg, mj, self.edge_threshold)
        if len(events) == 0 and len(switches) == 0:
            return None
        n_pp, n_pq, lists = ses.n_pp, ses.n_pq, N["lists"]
        ses.export(lists[:2 * n_pp].reshape(2, n_pp), lists[2 * n_pp:2 * (n_pp + n_pq)].reshape(2, n_pq))
        self._topo = (ses, None, None, None)   # (its lists are the ones to come: _install_event_topology)
        return events, switches, n_pp, n_pq

    def _upload_events(self, events, n_pp, n_pq):
        """The rewired junction coordinates and displacements, the live grains and the new lists back to the device,
        asynchronously; the lists go straight into the buffers the topology lives in while they fit
        (_install_topology_in_place finds them there).  Returns the new edge lists."""
        B, dev = self._evb, self.x["joint"].device
        self.x["joint"].copy_(B["xj"], non_blocking=True)
        self.pred["joint"].copy_(B["yj"], non_blocking=True)
        if len(events):
            B["np"]["live"][:] = self.mask["grain"][:, 0]
            self._live_grain.copy_(B["live"], non_blocking=True)
            if self._traj is not None:
                self._candidate_mask(B["np"]["cand"])
                self._cand_grain.copy_(B["cand"], non_blocking=True)
        C = self._cap
        if C is not None and n_pp <= C["cap"][ET_JJ] and n_pq <= C["cap"][JG] and n_pq <= C["cap"][GJ]:
            jj, jg = C["lists"][ET_JJ][:2 * n_pp].view(2, n_pp), C["lists"][JG][:2 * n_pq].view(2, n_pq)
            jj.copy_(B["lists"][:2 * n_pp].view(2, n_pp), non_blocking=True)
            jg.copy_(B["lists"][2 * n_pp:2 * (n_pp + n_pq)].view(2, n_pq), non_blocking=True)
            gj = C["lists"][GJ][:2 * n_pq].view(2, n_pq)
            torch.stack((jg[1], jg[0]), out=gj)
            return {ET_JJ: jj, JG: jg, GJ: gj}
        d = torch.empty(2 * (n_pp + n_pq), dtype=torch.int64, device=dev)
        d.copy_(B["lists"][:2 * (n_pp + n_pq)], non_blocking=True)
        jj, jg = d[:2 * n_pp].view(2, n_pp), d[2 * n_pp:].view(2, n_pq)
        return {ET_JJ: jj, JG: jg, GJ: torch.stack((jg[1], jg[0]))}

    def _install_event_topology(self, new_ei):
        """The rewired lists become the rollout's topology (_set_topology); the session that exported them follows them."""
        self._set_topology(new_ei, lasting=False, trusted=True)
        if self._topo is not None and self._topo[1] is None:
            jj, jg = self.edge_index[ET_JJ], self.edge_index[JG]
            self._topo = (self._topo[0], jj, jg, (jj._version, jg._version))

    def step(self):
        """Advance one rollout step; returns the prediction dict (tensors are reused)."""
        if self.steps_done % 16 == 0:
            self.refresh_weights()
        self._carry_home()
        if self._pipelined():
            self._ensure_edge_records()
        if self.use_graph:
            self._replay(1)
        else:
            self._enqueue_step()
        self.steps_done += 1
        return self.pred

    # steps per graph in run(): a graph-to-graph boundary costs ~10 us on the GPU (cfg3, 500 steps: 4 steps per graph 2 867
    # steps/s, 10 steps per graph 2 897); bench.py measures with this default
    RUN_UNROLL = 10

    def run(self, n_steps: int):
        """`n_steps` static-topology steps.  With hipGraph replay the bulk goes through a graph of
        RUN_UNROLL consecutive steps (same kernels, same order, same results as step() x n)."""
        self.refresh_weights()
        self._carry_home()
        if self.use_graph and n_steps >= self.RUN_UNROLL:
            if self._pipelined():
                self._ensure_edge_records()
            for _ in range(n_steps // self.RUN_UNROLL):
                self._replay(self.RUN_UNROLL)
            self.steps_done += n_steps - n_steps % self.RUN_UNROLL
            n_steps %= self.RUN_UNROLL
        for _ in range(n_steps):
            self.step()
        return self.pred

    def range_exceeded(self, clear=True) -> bool:
        """True when a fused cell has clamped an activation to fp16's range since the last check (include/ggnn.h,
        OPERAND RANGE): the trajectory since then is NOT the reference's -- re-run with GGNN_DEC=split GGNN_ENC=split.
        state() checks it (it synchronises anyway); one 4-byte read-back."""
        hit = self._range_hit   # (reports of run_events' committed steps, read with their event counts)
        if clear:
            self._range_hit = False
        return self.be.range_exceeded(self.x["joint"].device, clear, flag=self._range_word) or hit

    def state(self):
        """Final state a caller gathers across ranks: joint xy and grain (area, extraV).  Raises when the fused
        cells reported an operand beyond their arithmetic's range on the way here."""
        if self.range_exceeded():
            raise _lib.GGNNError("an activation reached fp16's range (+-65504) in a fused cell: this trajectory was computed "
                            "with clamped operands; re-run with GGNN_DEC=split GGNN_ENC=split (full fp32 range)")
        return {"joint_xy": self.x["joint"][:, :2].clone(), "grain_area_v": self.x["grain"][:, 3:5].clone()}

    def edge_attr_dict(self):
        if self.noflux:
            # the step's fused refresh writes the lengths of the forward's edges (the masked tables' slots); grain 0's
            # edges of the full lists get theirs here -- the same kernel expression, z clamp off
            off = torch.zeros(2, dtype=torch.int32, device=self.x["joint"].device)
            self.be.step_refresh(self.x["joint"], self.x["grain"], self.zmax, off, self._refresh_edges(self.edge_index))
        return {et: self.edge_attr[et].view(-1, 1) for et in EDGE_TYPES}
