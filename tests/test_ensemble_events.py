"""Events per trajectory of a disjoint-union rollout: topology.EnsembleSessions against the reference's recorded
updates, ggnn_detect_events_traj against numpy, GrainRollout.enable_events(traj_offsets=...) / trajectory_states() and
dist.rollout_trajectories(events=...) against the trajectories' own rollouts, bit for bit."""
import os
import socket

import numpy as np
import pytest
import torch

from helpers import EDGE_TYPES, GOLDEN, etk, load_graph, product_models, tt
from graingraphnn_amd import _lib, synthetic
from graingraphnn_amd.topology import (GJ, JG, JJ, EnsembleSessions, TopologyError, check_traj_offsets,
                                       union_edge_segments)

DEV = "cuda"
EV = dict(np.load(os.path.join(GOLDEN, "golden_cfg1_events.npz")))
SCENARIOS = ("elim1", "mass3", "mass4", "mixed", "switch1", "switch3")
AREA_THR, EDGE_THR = 1e-4, 0.6


def k(et):
    return "ei_" + "__".join(et)


# ---- CPU: the host side ----------------------------------------------------------------------------------------------------

def scenario_inputs(name, malformed=False):
    """One recorded call of the reference's Cmodel.update as a trajectory: its arrays, and predicted areas that make
    test.py:418-420 pick exactly the recorded candidates in the recorded order (everything else far above the threshold;
    one dead grain, where there is one, far below it: the live mask must keep it out)."""
    i = name + "__in_"
    ge = EV[i + "grain_event"].astype(np.int64)
    mg = EV[i + "mask_grain"].astype(np.int64).copy()
    area = np.ones(mg.shape[0], np.float32)
    area[ge] = (-1.0 + 1e-3 * np.arange(len(ge))).astype(np.float32)
    dead = np.flatnonzero(mg[:, 0] == 0)
    if len(dead):
        area[dead[0]] = -5.0
    pq = EV[i + k(JG)].copy()
    if malformed:   # tests/test_topology.py, test_invalid_lists_fail_loudly: grain 44 loses a corner
        pq[1, np.flatnonzero(pq[1] == 44)[0]] = 45
    return dict(xj=EV[i + "x_joint"].copy(), yj=EV[i + "y_joint"].copy(), yg=EV[i + "y_grain"].copy(), area=area,
                prob=torch.sigmoid(torch.from_numpy(EV[i + "edge_event"])).numpy(), mg=mg,
                mj=EV[i + "mask_joint"].astype(np.int64).copy(), pp=EV[i + k(JJ)].copy(), pq=pq)


def union_of(parts):
    off_g = np.concatenate([[0], np.cumsum([p["mg"].shape[0] for p in parts])]).astype(np.int64)
    off_j = np.concatenate([[0], np.cumsum([p["mj"].shape[0] for p in parts])]).astype(np.int64)
    cat = lambda key: np.ascontiguousarray(np.concatenate([p[key] for p in parts]))
    u = {key: cat(key) for key in ("xj", "yj", "yg", "area", "prob", "mg", "mj")}
    u["pp"] = np.concatenate([p["pp"] + off_j[t] for t, p in enumerate(parts)], axis=1)
    u["pq"] = np.concatenate([p["pq"] + np.array([[off_j[t]], [off_g[t]]]) for t, p in enumerate(parts)], axis=1)
    return u, off_g, off_j


def apply_union(ens, u, counts=None, ended=None):
    n = ens.n_traj
    counts = np.ones((n, 2), np.int32) if counts is None else counts
    return ens.apply(u["xj"], u["yj"], u["yg"][:, 0], u["prob"], u["area"], u["mg"], u["mj"], counts, ended, AREA_THR, EDGE_THR)


def assert_trajectory_is_golden(name, t, u, res, off_g, off_j, pp, pq):
    o = name + "__out_"
    g0, g1, j0, j1 = off_g[t], off_g[t + 1], off_j[t], off_j[t + 1]
    assert np.array_equal(pp - j0, EV[o + k(JJ)]), (name, "junction list, values or column order")
    assert np.array_equal(pq - np.array([[j0], [g0]]), EV[o + k(JG)]), (name, "junction-grain list")
    assert np.array_equal(u["mg"][g0:g1], EV[o + "mask_grain"]) and np.array_equal(u["mj"][j0:j1], EV[o + "mask_joint"]), name
    assert np.array_equal(u["xj"][j0:j1], EV[o + "x_joint"]) and np.array_equal(u["yj"][j0:j1], EV[o + "y_joint"]), name
    ev, sw = res["per_traj"].get(t, (np.zeros(0, np.int64), np.zeros((0, 2), np.int64)))
    assert np.array_equal(ev, EV[o + "grain_event"]) and np.array_equal(sw, EV[o + "switching_list"]), name


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4, 5), (4, 2, 5, 0, 3, 1)])
def test_ensemble_sessions_equal_the_reference_scenario_by_scenario(order):
    """The six recorded updates of the reference as six trajectories of ONE union: one apply gives every trajectory its own
    recorded result, bit for bit, and the union's lists are the concatenation in trajectory order."""
    names = [SCENARIOS[i] for i in order]
    u, off_g, off_j = union_of([scenario_inputs(n) for n in names])
    ens = EnsembleSessions(u["pp"], u["pq"], off_g, off_j)
    res = apply_union(ens, u)
    assert res["changed"] == list(range(6)) and not res["refused"]
    n_pp = [EV[n + "__out_" + k(JJ)].shape[1] for n in names]
    n_pq = [EV[n + "__out_" + k(JG)].shape[1] for n in names]
    assert res["n_pp"] == sum(n_pp) and res["n_pq"] == sum(n_pq)
    pp = res["lists"][:2 * res["n_pp"]].reshape(2, -1)
    pq = res["lists"][2 * res["n_pp"]:2 * (res["n_pp"] + res["n_pq"])].reshape(2, -1)
    seg_pp, seg_pq = np.concatenate([[0], np.cumsum(n_pp)]), np.concatenate([[0], np.cumsum(n_pq)])
    assert np.array_equal(ens.segments()[0], seg_pp) and np.array_equal(ens.segments()[1], seg_pq)
    events, switches = [], []
    for t, name in enumerate(names):
        assert_trajectory_is_golden(name, t, u, res, off_g, off_j, pp[:, seg_pp[t]:seg_pp[t + 1]], pq[:, seg_pq[t]:seg_pq[t + 1]])
        local = ens.local_lists(t)
        for et in (GJ, JG, JJ):
            assert np.array_equal(local[et], EV[name + "__out_" + k(et)]), (name, et)
        events.append(EV[name + "__out_grain_event"] + off_g[t])
        switches.append(EV[name + "__out_switching_list"].reshape(-1, 2) + off_j[t])
    assert np.array_equal(res["events"], np.concatenate(events)) and np.array_equal(res["switches"], np.concatenate(switches))
    # the new lists are again a disjoint union in trajectory order
    assert np.array_equal(union_edge_segments(pp, off_j, off_j), seg_pp)
    # a trajectory without candidates, and an ended one, are left alone
    u2, _, _ = union_of([scenario_inputs(n) for n in names])
    ens2 = EnsembleSessions(u2["pp"], u2["pq"], off_g, off_j)
    counts = np.ones((6, 2), np.int32)
    counts[1] = 0
    res2 = apply_union(ens2, u2, counts, ended=np.array([0, 0, 0, 1, 0, 0], np.int32))
    assert res2["changed"] == [0, 2, 4, 5]
    for t in (1, 3):
        i = names[t] + "__in_"
        assert np.array_equal(u2["mg"][off_g[t]:off_g[t + 1]], EV[i + "mask_grain"])
        assert np.array_equal(u2["xj"][off_j[t]:off_j[t + 1]], EV[i + "x_joint"])
        assert np.array_equal(ens2.local_lists(t)[JJ], EV[i + k(JJ)])


@pytest.mark.parametrize("bad_first", [True, False])
def test_refusal_is_local(bad_first):
    """A trajectory whose candidate grain has a malformed junction ring beside the recorded `mixed` update: the refusal is
    reported for that trajectory with its message, its slices and lists stay untouched, the other comes out as recorded."""
    parts = [scenario_inputs("elim1", malformed=True), scenario_inputs("mixed")]
    names = ["elim1", "mixed"]
    if not bad_first:
        parts, names = parts[::-1], names[::-1]
    bad, good = (0, 1) if bad_first else (1, 0)
    u, off_g, off_j = union_of(parts)
    before = {key: v.copy() for key, v in u.items()}
    ens = EnsembleSessions(u["pp"], u["pq"], off_g, off_j)
    with pytest.raises(TopologyError):   # (alone, the session refuses it)
        s = parts[bad]
        ens.sessions[bad].apply(s["xj"].copy(), s["yj"].copy(), s["yg"][:, 0], s["prob"], [44], s["mg"].copy(), s["mj"].copy(), EDGE_THR)
    res = apply_union(ens, u)
    assert list(res["refused"]) == [bad] and res["refused"][bad] and res["changed"] == [good]
    g0, g1, j0, j1 = off_g[bad], off_g[bad + 1], off_j[bad], off_j[bad + 1]
    for key, lo, hi in (("xj", j0, j1), ("yj", j0, j1), ("mj", j0, j1), ("mg", g0, g1), ("yg", g0, g1), ("area", g0, g1)):
        assert np.array_equal(u[key][lo:hi], before[key][lo:hi]), key
    local = ens.local_lists(bad)
    assert np.array_equal(local[JJ], parts[bad]["pp"]) and np.array_equal(local[JG], parts[bad]["pq"])
    pp = res["lists"][:2 * res["n_pp"]].reshape(2, -1)
    pq = res["lists"][2 * res["n_pp"]:2 * (res["n_pp"] + res["n_pq"])].reshape(2, -1)
    seg_pp, seg_pq = ens.segments()
    assert np.array_equal(pp[:, seg_pp[bad]:seg_pp[bad + 1]], parts[bad]["pp"] + j0)
    assert_trajectory_is_golden("mixed", good, u, res, off_g, off_j, pp[:, seg_pp[good]:seg_pp[good + 1]],
                                pq[:, seg_pq[good]:seg_pq[good + 1]])
    assert np.array_equal(res["events"], EV["mixed__out_grain_event"] + off_g[good])


def test_bad_offsets_and_lists_that_are_no_disjoint_union_raise():
    """What enable_events(traj_offsets=...) checks before it opens a session."""
    u, off_g, off_j = union_of([scenario_inputs("elim1"), scenario_inputs("mixed")])
    assert np.array_equal(union_edge_segments(u["pp"], off_j, off_j), [0, 708, 1416])
    assert np.array_equal(union_edge_segments(u["pq"], off_j, off_g), [0, 708, 1416])
    crossing = u["pp"].copy()
    crossing[1, 5] += 236                              # an edge from trajectory 0 into trajectory 1
    with pytest.raises(_lib.GGNNError, match="crosses"):
        union_edge_segments(crossing, off_j, off_j)
    with pytest.raises(_lib.GGNNError, match="crosses"):
        EnsembleSessions(crossing, u["pq"], off_g, off_j)
    swapped = np.concatenate([u["pp"][:, 708:], u["pp"][:, :708]], axis=1)   # the segments out of order
    with pytest.raises(_lib.GGNNError, match="trajectory order"):
        union_edge_segments(swapped, off_j, off_j)
    interleaved = u["pq"].copy()
    interleaved[:, [3, 900]] = interleaved[:, [900, 3]]
    with pytest.raises(_lib.GGNNError, match="trajectory order"):
        EnsembleSessions(u["pp"], interleaved, off_g, off_j)
    outside = u["pp"].copy()
    outside[0, 0] = 472
    with pytest.raises(_lib.GGNNError, match="outside"):
        union_edge_segments(outside, off_j, off_j)
    ok = {"grain": [0, 118, 236], "joint": [0, 236, 472]}
    og, oj = check_traj_offsets(ok, 236, 472)
    assert og.tolist() == ok["grain"] and oj.tolist() == ok["joint"]
    for bad in ({"grain": [0, 118, 236]}, {"grain": [0, 118, 236], "joint": [0, 472]}, {"grain": [1, 118, 236], "joint": ok["joint"]},
                {"grain": [0, 150, 118, 236], "joint": [0, 100, 236, 472]}, {"grain": [0, 118, 235], "joint": ok["joint"]}, [0, 118, 236]):
        with pytest.raises(_lib.GGNNError):
            check_traj_offsets(bad, 236, 472)


# ---- GPU: the detection kernel ------------------------------------------------------------------------------------------------

def detection_problem(sizes, edges_per_traj, ended, seed=5):
    """A hand-made union: `sizes[t]` grains and twice as many junctions per trajectory, `edges_per_traj[t]` directed junction
    edges inside trajectory t (segments in trajectory order), candidates on the first and last grain of every trajectory and
    on the first and last edge of every segment, (dst, src) twins with a high logit, dead grains below the threshold, an edge
    count on the device that is smaller than the capacity with stale candidates behind it."""
    rs = np.random.RandomState(seed)
    sizes, n_traj = np.asarray(sizes, np.int64), len(sizes)
    off_g = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    off_j = 2 * off_g
    n_g = int(off_g[-1])
    area = rs.uniform(0.01, 1.0, n_g).astype(np.float32)
    live = np.ones(n_g, np.int32)
    area[rs.rand(n_g) < 0.05] = -0.5                      # candidates in the interior
    dead = rs.rand(n_g) < 0.1
    area[dead] = -1.0                                     # dead grains below the threshold ...
    live[dead] = 0
    for t in range(n_traj):                               # ... but never the first and the last grain: candidates
        for g in {int(off_g[t]), int(off_g[t + 1]) - 1} if sizes[t] else ():
            area[g], live[g] = -0.25, 1
    src, dst, logit = [], [], []
    for t in range(n_traj):
        n_e, j0, nj = int(edges_per_traj[t]), int(off_j[t]), int(2 * sizes[t])
        assert n_e == 0 or nj >= 2
        s = rs.randint(0, max(nj, 1), n_e)
        d = (s + 1 + rs.randint(0, max(nj - 1, 1), n_e)) % max(nj, 1)
        lg = np.where(rs.rand(n_e) < 0.1, 3.0, -3.0).astype(np.float32)
        if n_e:
            for e in {0, n_e - 1}:                        # the first and the last edge of the segment: src < dst, high logit
                s[e], d[e], lg[e] = min(s[e], d[e]), max(s[e], d[e]), 4.0
        if n_e >= 4:                                      # a twin (dst, src) of the first edge with a high logit: not counted
            s[1], d[1], lg[1] = d[0], s[0], 4.0
        src.append(s + j0)
        dst.append(d + j0)
        logit.append(lg)
    src, dst, logit = np.concatenate(src), np.concatenate(dst), np.concatenate(logit)
    E, cap = len(src), len(src) + 300
    flat = rs.randint(0, max(int(off_j[-1]), 1), 2 * cap).astype(np.int64)   # (stale entries behind the live list [2, E])
    flat[:E], flat[E:2 * E] = src, dst
    edge_event = np.full(cap, 5.0, np.float32)            # stale candidates behind E
    edge_event[:E] = logit
    ended_words = np.zeros(n_traj, np.int32)
    ended_words[list(ended)] = 1
    # numpy: the counts
    counts = np.zeros((n_traj, 2), np.int64)
    tg = np.searchsorted(off_g, np.arange(n_g), side="right") - 1
    np.add.at(counts[:, 0], tg[(live > 0) & (area < np.float32(AREA_THR))], 1)
    te = np.searchsorted(off_j, src, side="right") - 1
    np.add.at(counts[:, 1], te[(logit > np.float32(0.4)) & (src < dst)], 1)
    return dict(area=area, live=live, flat=flat, edge_event=edge_event, E=E, cap=cap, off_g=off_g, off_j=off_j,
                ended=ended_words, counts=counts, n_traj=n_traj)


def run_detection(P, one_trajectory=False, with_ended=True, separate_buffers=False):
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    n = 1 if one_trajectory else P["n_traj"]
    off_g = d(P["off_g"][[0, -1]] if one_trajectory else P["off_g"])
    off_j = d(P["off_j"][[0, -1]] if one_trajectory else P["off_j"])
    if separate_buffers:
        flags, counts = torch.full((3,), 77, dtype=torch.int32, device=DEV), torch.full((n, 2), 77, dtype=torch.int32, device=DEV)
    else:
        buf = torch.full((3 + 2 * n,), 77, dtype=torch.int32, device=DEV)   # (the call zeroes what it counts into)
        flags, counts = buf[:3], buf[3:]
    word = torch.tensor([5], dtype=torch.int32, device=DEV)
    ended = d(P["ended"]) if with_ended and not one_trajectory else None
    ei = d(P["flat"]).view(2, P["cap"])
    be.detect_events_traj(d(P["area"]), d(P["live"]), AREA_THR, d(P["edge_event"]), ei, 0.4, off_g, off_j, counts, flags,
                          ended=ended, range_word=word, E_dev=torch.tensor([P["E"]], dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    return flags.cpu().numpy(), counts.view(n, 2).cpu().numpy(), int(word.cpu()[0])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["seven", "offsets_from_global_memory"])
def test_detection_kernel_against_numpy(case):
    """ggnn_detect_events_traj: exact counts per trajectory, totals over the running trajectories, the range word moved and
    cleared; trajectory boundaries inside waves and blocks; with one trajectory the totals of ggnn_detect_events."""
    from graingraphnn_amd.backend import default_backend
    if case == "seven":
        P = detection_problem([1, 63, 64, 65, 256, 257, 300], [2, 100, 0, 131, 500, 513, 601], ended=(2, 5))
    else:   # more trajectories than the kernel stages in LDS (511), empty ones among them
        rs = np.random.RandomState(9)
        sizes = rs.randint(0, 4, 700)
        sizes[[0, 699]] = 2
        P = detection_problem(sizes, np.where(sizes > 0, rs.randint(0, 5, 700), 0), ended=(0, 3, 350, 698))
    want = P["counts"].copy()
    assert (want[:, 0] > 0).sum() >= P["n_traj"] // 2 and (want[:, 1] > 0).sum() >= 5
    assert want[P["ended"] > 0].sum() > 0, "the ended trajectories must have candidates to leave out"
    running = want.copy()
    running[P["ended"] > 0] = 0
    for separate in (False, True):
        flags, counts, word = run_detection(P, separate_buffers=separate)
        assert np.array_equal(counts, running), (case, separate)
        assert flags.tolist() == [running[:, 0].sum(), running[:, 1].sum(), 5] and word == 0
    flags, counts, _ = run_detection(P, with_ended=False)
    assert np.array_equal(counts, want) and flags[:2].tolist() == want.sum(0).tolist()
    # one trajectory: the two words of ggnn_detect_events on the same inputs
    flags1, counts1, _ = run_detection(P, one_trajectory=True)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    single = torch.full((3,), 77, dtype=torch.int32, device=DEV)
    default_backend().detect_events(d(P["area"]), d(P["live"]), AREA_THR, d(P["edge_event"]), d(P["flat"]).view(2, P["cap"]),
                                    0.4, single, range_word=torch.tensor([5], dtype=torch.int32, device=DEV),
                                    E_dev=torch.tensor([P["E"]], dtype=torch.int64, device=DEV))
    assert flags1.tolist() == single.cpu().tolist() == [want[:, 0].sum(), want[:, 1].sum(), 5]
    assert counts1.tolist() == [flags1[:2].tolist()]


@pytest.mark.gpu
def test_detection_entry_point_validates_on_the_host():
    lib = _lib.load()
    buf = (torch.zeros(64, dtype=torch.int64, device=DEV))
    p = _lib.ptr(buf)
    args = lambda n_traj, skip: (p, p, 4, 0.0, p, p, 2, None, 0.0, p, p, n_traj, None, skip, p, p, None, None)
    assert lib.ggnn_detect_events_traj(*args(0, -1)) == -1          # no trajectory
    assert lib.ggnn_detect_events_traj(*args(2, 0)) == -1           # a skipped local grain: not supported yet
    assert lib.ggnn_detect_events_traj(None, None, 1, 0.0, None, None, 0, None, 0.0, None, None, 1, None, -1, None, None, None, None) == -1


# ---- GPU: rollouts --------------------------------------------------------------------------------------------------------------

QOI_KW = dict(patch_size=40.0, mesh_size=0.08, ini_height=2.0, final_height=50.0)


def cfg1(kind="fixture", seed=0, sigma=1e-3, dz=0.0):
    x, ei, ea = load_graph("40")
    if kind != "fixture":
        x = synthetic.perturbed_copy(x, sigma, seed)
    if dz:
        x = {nt: v.copy() for nt, v in x.items()}
        for nt in x:
            x[nt][:, 2] += np.float32(dz)
    return x, ei, ea


def rollout_of(graph, use_graph, qoi, traj_offsets=None):
    from graingraphnn_amd import GrainRollout
    R, Cm = product_models(10020, 1.0, DEV)
    X = tt(graph[0], DEV)
    ro = GrainRollout(R, Cm, X, tt(graph[1], DEV), tt(graph[2], DEV), 6, use_graph=use_graph, refresh_centres=True)
    n_g, n_j = X["grain"].size(0), X["joint"].size(0)
    ro.enable_events({"grain": np.ones((n_g, 1)), "joint": np.ones((n_j, 1))}, AREA_THR, EDGE_THR, **(
        {} if traj_offsets is None else {"traj_offsets": traj_offsets}))
    if qoi:
        ro.enable_qoi(capacity=40, **QOI_KW, **({} if traj_offsets is None else {"traj_offsets": traj_offsets["grain"]}))
    return ro, X


def snapshot(xj, xg, mask, lists, qoi=None):
    s = {"x_joint": xj.cpu().numpy().copy(), "x_grain": xg.cpu().numpy().copy(),
         "mask_grain": np.array(mask["grain"], copy=True), "mask_joint": np.array(mask["joint"], copy=True)}
    for et in EDGE_TYPES:
        s[etk(et)] = np.array(lists[et].cpu().numpy() if isinstance(lists[et], torch.Tensor) else lists[et], copy=True)
    if qoi is not None:
        s.update(qoi)
    return s


def qoi_rows(q, lo=None, hi=None, t=None):
    layers = q["layers"] if t is None else q["layers"][t]
    return {"volume": q["volume"][lo:hi].cpu().numpy().copy(), "size": q["size"][lo:hi].cpu().numpy().copy(), "layers": int(layers)}


def run_alone(graph, n_steps, use_graph=True, qoi=False):
    """A trajectory's own rollout: the state after every step_events(), its events, and where its update was refused:
    (steps: list of (state, events, switches), ended_at or None, the state it holds after the refusal or None)."""
    ro, X = rollout_of(graph, use_graph, qoi)
    steps = []
    for _ in range(n_steps):
        try:
            _, ev, sw = ro.step_events()
        except TopologyError as err:
            final = snapshot(X["joint"], X["grain"], ro.mask, ro.edge_index, qoi_rows(ro.qoi()) if qoi else None)
            return steps, ro.steps_done, final, str(err)
        steps.append((snapshot(X["joint"], X["grain"], ro.mask, ro.edge_index), ev.copy(), sw.copy()))
    final = snapshot(X["joint"], X["grain"], ro.mask, ro.edge_index, qoi_rows(ro.qoi()) if qoi else None)
    return steps, None, final, None


def assert_same_state(a, b, what):
    assert a.keys() >= b.keys() or b.keys() >= a.keys()
    for key in set(a) & set(b):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), (what, key)


def union_rollout(graphs, use_graph, qoi):
    x, ei, ea, slices = synthetic.disjoint_union(graphs)
    off = {nt: [s[nt][0] for s in slices] + [slices[-1][nt][1]] for nt in ("grain", "joint")}
    ro, X = rollout_of((x, ei, ea), use_graph, qoi, traj_offsets=off)
    return ro, X, slices


def state_of(ro, t, slices, with_qoi):
    st = ro.trajectory_states()[t]
    q = None
    if with_qoi:
        q = qoi_rows(ro.qoi(), *slices[t]["grain"], t)
    return snapshot(st["x_joint"], st["x_grain"], st["mask"], st["edge_index"], q), st


def check_union_against_own_rollouts(ro, slices, alone, n_steps, qoi, after_step=None):
    """`n_steps` of the union's step_events(): after every step every running trajectory equals its own rollout (rows of x,
    masks, local lists, events); a trajectory ends where its own rollout was refused, with what that one held.  Returns the
    number of (trajectory, step) comparisons of running trajectories made AFTER another trajectory had ended."""
    later = 0
    for step in range(n_steps):
        _, events, switches = ro.step_events()   # must not raise
        states = ro.trajectory_states()
        any_ended = any(a[1] is not None and a[1] <= step for a in alone)
        for t, (steps, ended_at, final, message) in enumerate(alone):
            (g0, g1), (j0, j1) = slices[t]["grain"], slices[t]["joint"]
            mine_ev = events[(events >= g0) & (events < g1)] - g0
            mine_sw = switches[(switches[:, 0] >= j0) & (switches[:, 0] < j1)] - j0
            if ended_at is not None and step >= ended_at:
                assert states[t]["ended_at"] == ended_at and states[t]["error"] == message, (t, step)
                assert len(mine_ev) == 0 and len(mine_sw) == 0, (t, step)
                got, _ = state_of(ro, t, slices, qoi)
                assert_same_state(got, final, f"trajectory {t}, ended at {ended_at}, seen after step {step}")
                continue
            assert states[t]["ended_at"] is None and states[t]["error"] is None, (t, step)
            want, want_ev, want_sw = steps[step]
            assert np.array_equal(mine_ev, want_ev) and np.array_equal(mine_sw, want_sw.reshape(-1, 2)), (t, step)
            assert_same_state(snapshot(states[t]["x_joint"], states[t]["x_grain"], states[t]["mask"], states[t]["edge_index"]),
                              want, f"trajectory {t} after step {step}")
            later += bool(any_ended)
        if after_step is not None:
            after_step(step, events, switches)
    return later


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
@torch.no_grad()
def test_union_equals_the_trajectories_own_rollouts_and_the_reference(use_graph):
    """Three cfg1 trajectories -- the fixture itself between two perturbed copies -- as one union with events per trajectory:
    after each of 5 steps every trajectory's rows of x, masks, local lists and events are those of its own GrainRollout, bit
    for bit; the middle one passes the assertions of test_event_rollout_reproduces_reference_trajectory; the segment graphs
    survive the events."""
    graphs = [cfg1("perturbed", 1000), cfg1(), cfg1("perturbed", 1001)]
    alone = [run_alone(g, 5, use_graph) for g in graphs]
    assert alone[1][1] is None, "the reference's cfg1 trajectory is refused at its sixth step, not before"
    ro, X, slices = union_rollout(graphs, use_graph, qoi=False)
    (g0, g1), (j0, j1) = slices[1]["grain"], slices[1]["joint"]
    seen = {}

    def middle_is_the_reference(step, events, switches):
        if use_graph:
            seen.setdefault("graphs", (ro._graph_fwd, ro._graph_ref))
            assert seen["graphs"][0] is ro._graph_fwd and seen["graphs"][1] is ro._graph_ref and ro._graph_fwd is not None
        st = ro.trajectory_states()[1]
        mine = events[(events >= g0) & (events < g1)] - g0
        if step + 1 < 3:
            assert len(mine) == 0
        elif step + 1 in (3, 4):
            name = f"mass{step + 1}"
            assert mine.tolist() == EV[name + "__out_grain_event"].tolist()
            for et in EDGE_TYPES:
                assert np.array_equal(st["edge_index"][et], EV[name + "__out_ei_" + etk(et)]), (step, et)
            assert np.array_equal(st["mask"]["grain"], EV[name + "__out_mask_grain"])
            assert np.array_equal(st["mask"]["joint"], EV[name + "__out_mask_joint"])
        if step + 1 == 4:
            assert st["edge_index"][JJ].shape[1] == 156 and int(st["mask"]["grain"].sum()) == 26
        # the union's lists: the concatenation of the trajectories' lists in trajectory order
        states = ro.trajectory_states()
        for et in EDGE_TYPES:
            shift = lambda t: np.array([[slices[t][et[0]][0]], [slices[t][et[-1]][0]]])
            cat = np.concatenate([states[t]["edge_index"][et] + shift(t) for t in range(3)], axis=1)
            assert np.array_equal(ro.edge_index[et].cpu().numpy(), cat), (step, et)

    check_union_against_own_rollouts(ro, slices, alone, 5, False, middle_is_the_reference)
    assert sum(len(e) for e in ro.grain_events) >= 97
    with pytest.raises(_lib.GGNNError, match="step_events"):
        ro.run_events(1)


# candidate perturbations of the cfg1 fixture for the test below: (kind, seed, sigma, shift of the initial z)
CANDIDATES = (("fixture", 0, 0.0, 0.0), ("perturbed", 1000, 1e-3, 0.0), ("perturbed", 7, 5e-3, 0.0),
              ("perturbed", 11, 2e-2, 0.0), ("fixture", 0, 0.0, 0.05), ("perturbed", 3, 1e-2, -0.03))
MAX_STEPS = 12


@pytest.mark.gpu
@torch.no_grad()
def test_a_trajectory_ends_and_the_ensemble_goes_on():
    """Three trajectories whose own rollouts are refused at steps that are not all equal (picked from CANDIDATES by running
    each alone first): the union does not raise, every trajectory ends where its own rollout did with the state, the volumes,
    sizes and layers that one held, the survivors keep matching their own rollouts, and once all have ended a step does no
    host rewiring.  Picked on the MI355X this was written on: see the printed line."""
    alone = {c: run_alone(cfg1(c[0], c[1], c[2], c[3]), MAX_STEPS, True, qoi=True) for c in CANDIDATES}
    ends = {c: a[1] for c, a in alone.items()}
    print("end steps of the candidates:", ends)
    ending = sorted((c for c in CANDIDATES if ends[c] is not None), key=lambda c: ends[c])
    assert len(ending) >= 3 and ends[ending[0]] < ends[ending[-1]], \
        f"no three candidates that end within {MAX_STEPS} steps at steps that are not all equal: {ends}"
    picked = [ending[len(ending) // 2], ending[0], ending[-1]]   # (the first to end stands in the middle of the union)
    if len({id(c) for c in picked}) < 3:
        picked = [ending[1], ending[0], ending[-1]]
    print("picked:", picked, "ending after", [ends[c] for c in picked], "completed steps")
    ro, X, slices = union_rollout([cfg1(*c) for c in picked], True, qoi=True)
    last = max(ends[c] for c in picked)
    later = check_union_against_own_rollouts(ro, slices, [alone[c] for c in picked], last + 1, True)
    assert later >= 1, "no step on which a trajectory ran on after another had ended"
    states = ro.trajectory_states()
    assert [s["ended_at"] for s in states] == [ends[c] for c in picked]
    assert ro._ens["ended"].cpu().tolist() == [1, 1, 1]
    # every trajectory has ended: the totals are zero, a step reaches no host rewiring and changes no ended state
    rewired, before = ro._ens["rewired"], [state_of(ro, t, slices, True)[0] for t in range(3)]
    for _ in range(2):
        _, events, switches = ro.step_events()
        assert ro._ev_host[:2].tolist() == [0, 0] and len(events) == 0 and len(switches) == 0
    assert ro._ens["rewired"] == rewired
    for t in range(3):
        assert_same_state(state_of(ro, t, slices, True)[0], before[t], f"ended trajectory {t}, two steps on")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _four():
    return [cfg1("perturbed", 1000), cfg1(), cfg1("perturbed", 1001), cfg1("perturbed", 1002)]


EVENTS_KW = dict(area_threshold=AREA_THR, edge_threshold=EDGE_THR)
DIST_STEPS = 6   # (the reference's cfg1 trajectory -- position 1 -- is refused at its sixth step: one trajectory ends)


def _gloo_worker(rank, world, port, out):
    import torch.distributed as dist
    from graingraphnn_amd.dist import rollout_trajectories
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    R, Cm = product_models(10020, 1.0, DEV)
    with torch.no_grad():
        res = rollout_trajectories(R, Cm, _four(), 6, DIST_STEPS, rank, world, DEV, refresh_centres=True,
                                   qoi=dict(QOI_KW, capacity=40), events=EVENTS_KW)
    if rank == 0:
        torch.save({key: v.cpu() for key, v in res.items()}, out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@torch.no_grad()
def test_rollout_trajectories_with_events(tmp_path):
    """dist.rollout_trajectories(events=..., qoi=...) on four trajectories: one process = a gloo world of two, bit for bit,
    and both = the trajectories' own rollouts (an ended one: what it held when its update was refused)."""
    import torch.multiprocessing as mp
    from graingraphnn_amd.dist import rollout_trajectories
    graphs = _four()
    R, Cm = product_models(10020, 1.0, DEV)
    single = rollout_trajectories(R, Cm, graphs, 6, DIST_STEPS, 0, 1, DEV, refresh_centres=True, qoi=dict(QOI_KW, capacity=40),
                                  events=EVENTS_KW)
    assert set(single) == {"joint_xy", "grain_area_v", "volume", "size", "grain_live", "joint_live", "ended_at", "n_eliminated"}
    assert single["ended_at"].shape == (4,) and single["grain_live"].shape == (4, 118) and single["joint_live"].shape == (4, 236)
    assert all(v.dtype == torch.float32 for v in single.values())
    for t, g in enumerate(graphs):
        _, ended_at, final, _ = run_alone(g, DIST_STEPS, True, qoi=True)
        assert int(single["ended_at"][t]) == (-1 if ended_at is None else ended_at), t
        want = {"joint_xy": final["x_joint"][:, :2], "grain_area_v": final["x_grain"][:, 3:5], "volume": final["volume"],
                "size": final["size"], "grain_live": (final["mask_grain"][:, 0] > 0).astype(np.float32),
                "joint_live": (final["mask_joint"][:, 0] > 0).astype(np.float32),
                "n_eliminated": np.float32(118 - int((final["mask_grain"] > 0).sum()))}
        for key, v in want.items():
            assert np.array_equal(single[key][t].cpu().numpy(), v, equal_nan=True), (t, key)
    assert int(single["ended_at"][1]) == 5 and float(single["n_eliminated"].min()) > 0
    out = str(tmp_path / "gathered.pt")
    mp.spawn(_gloo_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = torch.load(out)
    assert set(got) == set(single)
    for key, v in single.items():
        assert torch.equal(got[key], v.cpu()), key


class _CountingLib:
    """The library with every call of an entry point noted (as in tests/test_qoi.py)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("ggnn_"):
            return fn

        def noted(*args):
            self.calls.append(name)
            return fn(*args)
        return noted


# The C-ABI calls the rollout's backend makes in one step_events() on the cfg1 fixture (eager launches, grain centres
# refreshed) behind the two forwards, as counted on the commit before the per-trajectory layer: a quiet step, and an eventful
# one (the session's own calls go through topology.py's handle of the library and are not among them).  The forwards in
# front of them (five calls under the default plans at this size) follow GGNN_DEC / GGNN_ENC.
QUIET_STEP = ["ggnn_heads_regressor", "ggnn_heads_classifier", "ggnn_step_update", "ggnn_detect_events", "ggnn_grain_centres",
              "ggnn_step_refresh"]
EVENTFUL_STEP = QUIET_STEP[:4] + ["ggnn_build_csr_batch"] + QUIET_STEP[4:]


@pytest.mark.gpu
@torch.no_grad()
def test_off_means_off():
    """Without traj_offsets a step_events() loop never reaches ggnn_detect_events_traj and makes, step for step, the C-ABI
    calls it made before the per-trajectory layer existed; with traj_offsets (one trajectory) the only difference is the
    detection entry point, and the state comes out bit-equal.  rollout_trajectories(events=None): the keys and bits of the
    static union."""
    from graingraphnn_amd import GrainRollout
    from graingraphnn_amd.backend import default_backend
    from graingraphnn_amd.dist import rollout_trajectories
    be = default_backend()

    def counted(traj_offsets):
        ro, _ = rollout_of(cfg1(), False, False, traj_offsets)
        ro.step_events()
        lib, per_step = be.lib, []
        try:
            for _ in range(4):
                be.lib = counting = _CountingLib(lib)
                ro.step_events()
                per_step.append(counting.calls)
        finally:
            be.lib = lib
        return per_step, ro
    off, ro_off = counted(None)
    print("entry points per step without traj_offsets:", off)
    assert ro_off._ens is None and [len(e) > 0 for e in ro_off.grain_events] == [False, False, True, True, True]
    n_fwd = off[0].index("ggnn_heads_regressor")
    assert n_fwd >= 2 and off[0][0] == "ggnn_edge_prepare" and all(c[:n_fwd] == off[0][:n_fwd] for c in off)
    assert [c[n_fwd:] for c in off] == [QUIET_STEP, EVENTFUL_STEP, EVENTFUL_STEP, EVENTFUL_STEP]   # steps 2-5
    on, ro_on = counted({"grain": [0, 118], "joint": [0, 236]})
    swap = lambda calls: ["ggnn_detect_events_traj" if c == "ggnn_detect_events" else c for c in calls]
    assert on == [swap(c) for c in off]
    for nt in ("joint", "grain"):
        assert torch.equal(ro_on.x[nt], ro_off.x[nt]), nt
    # events=None: the static union, as before
    graphs = [cfg1("perturbed", 1000), cfg1("perturbed", 1001)]
    R, Cm = product_models(10020, 1.0, DEV)
    res = rollout_trajectories(R, Cm, graphs, 6, 3, 0, 1, DEV)
    assert set(res) == {"joint_xy", "grain_area_v"}
    res = rollout_trajectories(R, Cm, graphs, 6, 3, 0, 1, DEV, qoi=QOI_KW, events=None)
    assert set(res) == {"joint_xy", "grain_area_v", "volume", "size"}
    for t, g in enumerate(graphs):
        X = tt(g[0], DEV)
        one = GrainRollout(R, Cm, X, tt(g[1], DEV), tt(g[2], DEV), 6, use_graph=True)
        one.enable_qoi(**QOI_KW)
        one.run(3)
        q = one.qoi()
        assert torch.equal(res["joint_xy"][t], X["joint"][:, :2]) and torch.equal(res["grain_area_v"][t], X["grain"][:, 3:5]), t
        assert torch.equal(res["volume"][t], q["volume"]) and torch.equal(res["size"][t], q["size"]), t


@pytest.mark.gpu
def test_refused_combinations_and_bad_unions_raise():
    from graingraphnn_amd import GrainRollout
    from test_noflux import fixture, initial_state
    f = fixture("noflux_40_seed1")
    R, Cm = product_models(int(f["weight_seed"]), 1.0, DEV)
    X, EI, EA, off, factor = initial_state(f, DEV)
    ro = GrainRollout(R, Cm, X, EI, EA, int(f["span"]), refresh_centres=True, domain_factor=factor, boundary="noflux",
                      max_y=float(f["max_y"]))
    with pytest.raises(_lib.GGNNError, match="noflux"):
        ro.enable_events({"grain": f["mask_grain"], "joint": f["mask_joint"]}, 1e-4, 0.6,
                         traj_offsets={"grain": [0, X["grain"].size(0)], "joint": [0, X["joint"].size(0)]})
    x, ei, ea, slices = synthetic.disjoint_union([cfg1(), cfg1("perturbed", 1000)])
    ei = {et: v.copy() for et, v in ei.items()}
    ei[JJ][1, 5] += 236   # an edge into the other trajectory
    R, Cm = product_models(10020, 1.0, DEV)
    ro = GrainRollout(R, Cm, tt(x, DEV), tt(ei, DEV), tt(ea, DEV), 6)
    mask = {"grain": np.ones((236, 1)), "joint": np.ones((472, 1))}
    with pytest.raises(_lib.GGNNError, match="crosses"):
        ro.enable_events(mask, 1e-4, 0.6, traj_offsets={"grain": [0, 118, 236], "joint": [0, 236, 472]})
    with pytest.raises(_lib.GGNNError):
        ro.enable_events(mask, 1e-4, 0.6, traj_offsets={"grain": [0, 118, 236], "joint": [0, 236, 471]})
    with pytest.raises(_lib.GGNNError, match="traj_offsets"):
        ro.trajectory_states()
