"""The (G, R) schedule on the device: generator.reference_gr_schedule against the reference's own lists, the table's
rounding, set_process_schedule's validation, ggnn_process_schedule against the numpy restatement of tests/schedcheck.py bit
for bit, and GrainRollout.set_process_schedule in step() / run() / step_events() / run_events(), on unions, with the QoI and
through dist.rollout_trajectories against rollouts that write the parameters from the host between steps."""
import ctypes
import os

import numpy as np
import pytest
import torch

import schedcheck
from helpers import EDGE_TYPES, GOLDEN, assert_close, load_graph, oracle, oracle_models, product_models, tt
from graingraphnn_amd import _lib, synthetic

DEV = "cuda"
PLANS = {"overlapped": dict(joint_launches=False, concurrent=True), "joint": dict(joint_launches=True, concurrent=True),
         "single": dict(joint_launches=False, concurrent=False)}


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_reference_gr_schedule_equals_the_reference_bit_for_bit():
    from graingraphnn_amd.generator import reference_gr_schedule
    d = np.load(os.path.join(GOLDEN, "gr_schedule.npz"))
    assert len(d["seeds"]) == 3 and any(int(f) == 2 ** (int(s) % 10) for s, f in zip(d["seeds"], d["freqs"]))
    for i, (seed, freq) in enumerate(zip(d["seeds"], d["freqs"])):
        G, R = reference_gr_schedule(int(seed), int(freq), float(d["ini_height"]), float(d["final_height"]), float(d["delta_z"]))
        assert G.dtype == R.dtype == np.float64 and len(G) == 20
        assert np.array_equal(G, d[f"G_{i}"]) and np.array_equal(R, d[f"R_{i}"]), (seed, freq)


def test_table_is_rounded_once_from_float64():
    from graingraphnn_amd.rollout import process_schedule_table
    rs = np.random.RandomState(0)
    G, R = rs.uniform(0.5, 10.0, (9, 3)), rs.uniform(0.2, 2.0, (9, 3))
    table, shared = process_schedule_table(G, R)
    assert table.dtype == np.float32 and table.shape == (9, 3, 2) and not shared
    assert np.array_equal(table[..., 0], np.float32(1 - G / 10)) and np.array_equal(table[..., 1], np.float32(R / 2))
    # ... which is not what rounding G first gives: the float64 arithmetic is part of the contract
    assert not np.array_equal(table[..., 0], np.float32(1) - np.float32(G) / np.float32(10))
    one, shared = process_schedule_table(G[:, 0], R[:, 0])
    assert shared and np.array_equal(one[:, 0], table[:, 0])
    # what the reference's assignment leaves in a float32 tensor
    x = torch.zeros(1, 5)
    x[:, 3], x[:, 4] = 1 - G[4, 1] / 10, R[4, 1] / 2
    assert np.array_equal(x[0, 3:5].numpy(), table[4, 1])
    feats = rs.uniform(-1, 1, (4, 2)).astype(np.float32)
    assert np.array_equal(process_schedule_table(features=feats)[0][:, 0], feats)
    assert process_schedule_table(features=feats[:, None, :].repeat(2, 1))[0].shape == (4, 2, 2)


def _bare_rollout(n_joint=10, noflux_union=False):
    """A GrainRollout with only what set_process_schedule's validation reads (it raises before the device is touched)."""
    from graingraphnn_amd import GrainRollout
    ro = object.__new__(GrainRollout)
    ro.n_nodes, ro.noflux, ro._traj, ro._sched = {"joint": n_joint, "grain": 6}, noflux_union, None, None
    if noflux_union:
        ro._traj = {"grain": np.array([0, 2, 6]), "joint": np.array([0, 4, n_joint])}
    return ro


def test_validation_errors():
    E = _lib.GGNNError
    ro = _bare_rollout()
    G, R = np.linspace(1, 2, 5), np.linspace(0.3, 0.4, 5)
    feats = np.zeros((5, 2), np.float32)
    for kw in (dict(), dict(G=G), dict(R=R), dict(G=G, R=R, features=feats), dict(G=G, features=feats)):
        with pytest.raises(E, match="not both and not neither"):
            ro.set_process_schedule(**kw)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(E, match="finite"):
            ro.set_process_schedule(np.where(np.arange(5) == 2, bad, G), R)
        with pytest.raises(E, match="finite"):
            ro.set_process_schedule(features=np.where(np.arange(10).reshape(5, 2) == 7, bad, feats))
    with pytest.raises(E, match="same shape"):
        ro.set_process_schedule(G, R[:4])
    with pytest.raises(E, match="same shape"):
        ro.set_process_schedule(G.reshape(5, 1, 1), R.reshape(5, 1, 1))
    with pytest.raises(E, match="features must be"):
        ro.set_process_schedule(features=np.zeros((5, 3)))
    with pytest.raises(E, match="at least one row"):
        ro.set_process_schedule(G[:0], R[:0])
    # shapes against the offsets
    G2, R2 = np.stack([G, G], 1), np.stack([R, R], 1)
    with pytest.raises(E, match="needs traj_offsets"):
        ro.set_process_schedule(G2, R2)
    with pytest.raises(E, match="2 trajectories, the offsets 3"):
        ro.set_process_schedule(G2, R2, traj_offsets={"joint": [0, 3, 3, 10]})
    for off in ([1, 4, 10], [0, 4, 9], [0, 6, 4, 10], [0]):
        with pytest.raises(E, match="rise from 0"):
            ro.set_process_schedule(G2, R2, traj_offsets={"joint": off})
    with pytest.raises(E, match="traj_offsets must be"):
        ro.set_process_schedule(G2, R2, traj_offsets={"grain": [0, 2, 6]})
    # a no-flux union has the constructor's offsets and no others
    nf = _bare_rollout(noflux_union=True)
    with pytest.raises(E, match="differ"):
        nf.set_process_schedule(G2, R2, traj_offsets={"joint": [0, 5, 10]})
    with pytest.raises(E, match="differ"):
        nf.set_process_schedule(G2, R2, traj_offsets={"grain": [0, 3, 6], "joint": [0, 4, 10]})
    with pytest.raises(E, match="3 trajectories, the offsets 2"):
        nf.set_process_schedule(np.stack([G] * 3, 1), np.stack([R] * 3, 1))
    single = _bare_rollout()
    single.noflux = True
    with pytest.raises(E, match="at construction"):
        single.set_process_schedule(G2, R2, traj_offsets={"grain": [0, 2, 6], "joint": [0, 4, 10]})
    # one way to do each
    ro._sched = {}
    with pytest.raises(E, match="clear_process_schedule"):
        ro.set_process_parameters(1.0, 1.0)
    ro._sched = None
    ro._enqueue_schedule()   # off: no launch, nothing touched (the object has no backend at all)


def test_entry_point_validates_on_the_host():
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda x=p, n=4, ldx=8, tab=p, rows=2, traj=1, off=None, si=p, so=p, sy=p: \
        lib.ggnn_process_schedule(x, n, ldx, tab, rows, traj, off, si, so, sy, None)
    for kw in (dict(x=None), dict(tab=None), dict(si=None), dict(so=None), dict(sy=None), dict(rows=0), dict(traj=0),
               dict(ldx=4), dict(n=0), dict(traj=2)):
        assert call(**kw) == -1, kw
    assert "ggnn_process_schedule" in _lib.EXPORTED_SYMBOLS and _lib.GGNN_ABI_VERSION == 26


def test_the_restatement_on_a_case_worked_by_hand():
    """Two trajectories of 2 and 1 junctions with an empty one between them, counter 0 -> row 1."""
    x = np.arange(24, dtype=np.float32).reshape(3, 8)
    table = np.array([[[.1, .2], [.3, .4], [.5, .6]], [[1.1, 1.2], [1.3, 1.4], [1.5, 1.6]]], np.float32)
    got, k = schedcheck.restate(x, table, [0, 2, 2, 3], 0)
    want = x.copy()
    want[:, 3:5] = np.float32([[1.1, 1.2], [1.1, 1.2], [1.5, 1.6]])
    assert k == 1 and np.array_equal(got, want)
    assert np.array_equal(schedcheck.restate(x, table, [0, 2, 2, 3], 5)[0], want)          # past the end: the last row
    assert np.array_equal(schedcheck.restate(x, table, [0, 2, 2, 3], -9)[0][:, 3:5], np.float32([[.1, .2], [.1, .2], [.5, .6]]))


@pytest.mark.parametrize("variant", schedcheck.VARIANTS)
def test_the_comparison_rejects_each_named_mistake(variant):
    """On the problems of the kernel tests the bit-for-bit comparison fails for every mistake the restatement can make on
    purpose, on the case that is there for it; the right answer passes the same comparison."""
    whole, table, off = schedcheck.problem(schedcheck.UNION_SIZES, 4, pad=3)
    G = schedcheck.GUARD
    x = whole[G:-G]
    counter = {"row_k": 0, "no_clamp": 4 + 7, "prev_traj": 1, "col2": 1, "col5": 1}[variant]
    right, k = schedcheck.restate(x, table, off, counter)
    wrong, _ = schedcheck.restate(x, table, off, counter, variant)
    assert k == counter + 1 and not np.array_equal(right, wrong), variant
    # the right answer, written out independently: junction by junction
    want = x.copy()
    r = min(max(counter + 1, 0), 3)
    for t in range(len(off) - 1):
        want[off[t]:off[t + 1], 3:5] = table[r, t]
    assert np.array_equal(right, want)
    if variant == "prev_traj":   # only the first junctions of the trajectories behind the first differ
        rows = np.flatnonzero((right != wrong).any(1))
        assert set(rows) <= set(off[1:-1].tolist()) and len(rows) >= 4


# ---- GPU: the kernel alone ---------------------------------------------------------------------------------------------------

def launch(whole, table, off, counter, alias=True):
    """One launch through the backend on the middle rows of `whole`: (whole after, step_out, step_in after, sync word)."""
    from graingraphnn_amd.backend import default_backend
    G = schedcheck.GUARD
    w = torch.from_numpy(whole.copy()).to(DEV)
    words = torch.tensor([counter, -12345, 0], dtype=torch.int32, device=DEV)
    step_in, step_out = words[:1], words[:1] if alias else words[1:2]
    default_backend().process_schedule(w[G:w.size(0) - G], torch.from_numpy(table).to(DEV),
                                       None if off is None else torch.from_numpy(off).to(DEV), step_in, step_out, words[2:])
    words = words.cpu().numpy()
    return w.cpu().numpy(), int(words[0] if alias else words[1]), int(words[0]), int(words[2])


def check_launch(sizes, n_rows, counter, pad, alias):
    whole, table, off = schedcheck.problem(sizes, n_rows, pad)
    G = schedcheck.GUARD
    want = whole.copy()
    want[G:-G], k = schedcheck.restate(whole[G:-G], table, off, counter)
    got, step_out, step_in, sync = launch(whole, table, off, counter, alias)
    what = (sizes if np.isscalar(sizes) else len(sizes), n_rows, counter, pad, alias)
    assert np.array_equal(got, want), what           # columns 3 and 4 only: every sentinel, padding and guard row intact
    assert step_out == k == counter + 1 and sync == 0 and step_in == (k if alias else counter), what


@pytest.mark.gpu
@pytest.mark.parametrize("n_joint", [1, 255, 256, 257, 1000])
def test_kernel_one_trajectory(n_joint):
    """NULL offsets; one block and several; both strides; the counter aliased and not; every clamp."""
    for pad in (0, 3):
        for alias in (True, False):
            check_launch(n_joint, 5, 1, pad, alias)
    for n_rows, counters in ((1, (-5, 0, 7)), (6, (-5, 0, 6 - 2, 6 - 1, 6 + 7))):
        for counter in counters:
            check_launch(n_joint, n_rows, counter, 3, counter % 2 == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["union", "more_offsets_than_lds"])
def test_kernel_union(case):
    sizes = schedcheck.UNION_SIZES if case == "union" else schedcheck.many_small()
    assert case == "union" or len(sizes) == 600
    for pad in (0, 3):
        for alias in (True, False):
            check_launch(sizes, 4, 1, pad, alias)
    for n_rows, counters in ((1, (-5, 0, 7)), (4, (-5, 0, 4 - 2, 4 - 1, 4 + 7))):
        for counter in counters:
            check_launch(sizes, n_rows, counter, 3, True)


@pytest.mark.gpu
def test_captured_launches_continue_the_counter():
    """A hipGraph of three launches on one counter word, each writing an array of its own: the first replay writes rows 1-3,
    the second rows 4-6 and leaves the counter at 6."""
    from graingraphnn_amd import GrainRollout
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    whole, table, off = schedcheck.problem(schedcheck.UNION_SIZES, 8)
    x0 = whole[schedcheck.GUARD:-schedcheck.GUARD]
    xs = [torch.from_numpy(x0.copy()).to(DEV) for _ in range(3)]
    tab, offs = torch.from_numpy(table).to(DEV), torch.from_numpy(off).to(DEV)
    words = torch.zeros(2, dtype=torch.int32, device=DEV)
    g = GrainRollout._captured(lambda: [be.process_schedule(x, tab, offs, words[:1], words[:1], words[1:]) for x in xs])
    assert words.cpu().tolist() == [0, 0]   # (a capture records, it does not run)
    for replay in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert words.cpu().tolist() == [3 * (replay + 1), 0]
        for i, x in enumerate(xs):
            want, _ = schedcheck.restate(x0, table, off, 3 * replay + i)
            assert np.array_equal(x.cpu().numpy(), want), (replay, i)


# ---- GPU: rollouts -----------------------------------------------------------------------------------------------------------

def schedule_rows(n_rows, n_traj=None, seed=5):
    rs = np.random.RandomState(seed)
    shape = (n_rows,) if n_traj is None else (n_rows, n_traj)
    return rs.uniform(0.5, 10.0, shape), rs.uniform(0.2, 2.0, shape)


def rollout(graph, plan="overlapped", use_graph=True, seed=31, **kw):
    from graingraphnn_amd import GrainRollout
    R, Cm = product_models(seed, 1.0, DEV)
    X = tt(graph[0], DEV)
    return GrainRollout(R, Cm, X, tt(graph[1], DEV), tt(graph[2], DEV), 6, use_graph=use_graph, **PLANS[plan], **kw), X


def clone(d):
    return {k: v.clone() for k, v in d.items()}


def assert_equal_dicts(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


STATIC_ROWS = 13   # one RUN_UNROLL graph and a remainder


@pytest.fixture(scope="module")
def static_oracle():
    """The oracle stepping the 13 rows on the CPU, once: the predictions of its last step."""
    G, Rp = schedule_rows(STATIC_ROWS)
    x, ei, ea = load_graph("40")
    oR, oC = oracle_models(31, 1.0)
    oX, oEI, oEA = tt(x), tt(ei), tt(ea)
    with torch.no_grad():
        for k in range(STATIC_ROWS):
            oX["joint"][:, 3], oX["joint"][:, 4] = 1.0 - G[k] / 10.0, Rp[k] / 2.0
            opred, oEA = oracle.rollout_step(oR, oC, oX, oEI, oEA, 6)
    return opred, oX


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("plan", list(PLANS))
@torch.no_grad()
def test_run_with_a_schedule_equals_host_writes_between_steps(plan, use_graph, static_oracle):
    """13 rows -- one RUN_UNROLL graph and a remainder -- through run(13) with the schedule on the device against 13 x
    (set_process_parameters(row) + step()) on a second rollout: x and the five prediction tensors bit for bit, the last
    step's predictions within the project's bar of the oracle stepping the same rows; three steps past the table hold the
    last row; the method again restarts at row 0 and, for a table of the same shape, keeps the captured graphs."""
    from graingraphnn_amd import GrainRollout
    assert STATIC_ROWS > GrainRollout.RUN_UNROLL and STATIC_ROWS % GrainRollout.RUN_UNROLL
    G, Rp = schedule_rows(STATIC_ROWS)
    graph = load_graph("40")
    a, Xa = rollout(graph, plan, use_graph)
    assert a._pipelined() == (plan == "overlapped")
    a.set_process_schedule(G, Rp)
    pa = clone(a.run(STATIC_ROWS))
    b, Xb = rollout(graph, plan, use_graph)
    for k in range(STATIC_ROWS):
        b.set_process_parameters(G[k], Rp[k])
        pb = b.step()
    assert_equal_dicts(Xa, Xb, "x after the last row")
    assert_equal_dicts(pa, clone(pb), "predictions of the last row")
    assert len(pa) == 5
    assert np.array_equal(Xa["joint"][:, 3:5].cpu().numpy(),
                          np.broadcast_to(np.float32([1 - G[-1] / 10, Rp[-1] / 2]), (236, 2)))
    opred, oX = static_oracle
    for k in pa:
        assert_close(pa[k], opred[k], f"{plan} graph={use_graph} {k}")
    for nt in Xa:
        assert_close(Xa[nt], oX[nt], f"{plan} graph={use_graph} x {nt}")
    # past the table the last row holds
    a.run(3)
    for _ in range(3):
        b.step()
    assert_equal_dicts(Xa, Xb, "x three steps past the table")
    assert a.steps_done == b.steps_done == STATIC_ROWS + 3
    with pytest.raises(_lib.GGNNError, match="clear_process_schedule"):
        a.set_process_parameters(1.0, 1.0)
    # the method again, mid-rollout: row 0 again; a table of the same shape keeps the captured graphs
    graphs = a._graphs
    G2, R2 = schedule_rows(STATIC_ROWS, seed=6)
    a.set_process_schedule(G2, R2)
    assert a._graphs is graphs
    a.run(2)
    for k in range(2):
        b.set_process_parameters(G2[k], R2[k])
        b.step()
    b.set_process_parameters(G2[2], R2[2])   # (the schedule's tail has written the row of the step to come)
    assert_equal_dicts(Xa, Xb, "x two steps into a second schedule")
    a.set_process_schedule(G2[:5], R2[:5])
    assert a._graphs is None and a._sched["table"].shape == (5, 1, 2)


def _perturbed(n, graph=None):
    x, ei, ea = graph or load_graph("40")
    return [(synthetic.perturbed_copy(x, 1e-3, 1000 + t), ei, ea) for t in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", ["periodic", "noflux"])
@torch.no_grad()
def test_union_with_a_schedule_per_trajectory(boundary):
    """Three perturbed trajectories, three schedules, one union: every trajectory's rows are its own rollout's."""
    steps = 5
    G, Rp = schedule_rows(steps, 3)
    if boundary == "periodic":
        graphs = _perturbed(3)
        x, ei, ea, slices = synthetic.disjoint_union(graphs)
        ro, X = rollout((x, ei, ea), refresh_centres=True)
        off = {nt: [s[nt][0] for s in slices] + [slices[-1][nt][1]] for nt in ("grain", "joint")}
        ro.set_process_schedule(G, Rp, traj_offsets={"joint": off["joint"]})
        alone = lambda g: rollout(g, refresh_centres=True)
    else:
        from test_noflux import fixture
        from test_noflux_ensemble import F40, nf_graph, nf_rollout
        d = fixture(F40)
        graphs = [nf_graph(d, 1000 + t, 2e-3) for t in range(3)]
        ro, X, slices = nf_rollout(d, graphs, True, events=False)
        assert ro._traj is not None
        ro.set_process_schedule(G, Rp)
        alone = lambda g: nf_rollout(d, [g], True, events=False, union=False)[:2]
    ro.run(steps)
    for t, g in enumerate(graphs):
        one, X1 = alone(g)
        one.set_process_schedule(G[:, t], Rp[:, t])
        one.run(steps)
        (g0, g1), (j0, j1) = slices[t]["grain"], slices[t]["joint"]
        assert torch.equal(X["joint"][j0:j1], X1["joint"]) and torch.equal(X["grain"][g0:g1], X1["grain"]), t
        assert np.array_equal(X1["joint"][0, 3:5].cpu().numpy(), np.float32([1 - G[-1, t] / 10, Rp[-1, t] / 2]))
    assert not torch.equal(X["joint"][slices[0]["joint"][0]:slices[0]["joint"][1], 3:5],
                           X["joint"][slices[1]["joint"][0]:slices[1]["joint"][1], 3:5])


EVENT_STEPS = 5
EVENT_KW = dict(refresh_centres=True, seed=10020)
MASK = {"grain": np.ones((118, 1)), "joint": np.ones((236, 1))}


def event_features():
    """Rows 0-2: the fixture's own parameters (its third step eliminates grains:
    test_speculative_event_loop_equals_step_events); later rows differ in the last bits that matter."""
    xj = load_graph("40")[0]["joint"]
    assert (xj[:, 3:5] == xj[0, 3:5]).all()
    feats = np.repeat(xj[:1, 3:5].astype(np.float32), EVENT_STEPS, axis=0)
    feats[3:] *= np.float32(1.0 + 1e-3) ** np.arange(1, EVENT_STEPS - 2, dtype=np.float32)[:, None]
    assert len(np.unique(feats[2:, 0])) == EVENT_STEPS - 2
    return feats


def event_state(ro, X, events, switches):
    s = {"x_" + nt: X[nt].cpu().numpy().copy() for nt in X}
    s.update({"mask_" + k: np.array(v, copy=True) for k, v in ro.mask.items()})
    s.update({"ei_" + "__".join(et): ro.edge_index[et].cpu().numpy().copy() for et in EDGE_TYPES})
    s.update({"ea_" + "__".join(et): ro.edge_attr_dict()[et].cpu().numpy().copy() for et in EDGE_TYPES})
    s.update({"p_" + k: ro.pred[k].cpu().numpy().copy() for k in ("joint", "grain", "grain_area")})
    s["events"] = np.concatenate([np.asarray(e).ravel() for e in events] + [[-1], [len(e) for e in events]])
    s["switches"] = np.concatenate([np.asarray(w).ravel() for w in switches] + [[-1], [len(w) for w in switches]])
    return s


@pytest.fixture(scope="module")
def event_reference():
    """step_events() with the row of every step written from the host in front of it, once."""
    feats = event_features()
    with torch.no_grad():
        ro, X = rollout(load_graph("40"), **EVENT_KW)
        ro.enable_events(MASK, 1e-4, 0.6)
        ev, sw = [], []
        for k in range(EVENT_STEPS):
            X["joint"][:, 3:5] = torch.from_numpy(feats[k]).to(DEV)
            _, e, w = ro.step_events()
            ev.append(e)
            sw.append(w)
        torch.cuda.synchronize()
    eventful = [len(e) > 0 or len(w) > 0 for e, w in zip(ev, sw)]
    assert eventful[2] and any(eventful) and not all(eventful), eventful   # (a condition on the input)
    return event_state(ro, X, ev, sw), eventful


def assert_same_event_state(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
@torch.no_grad()
def test_step_events_with_a_schedule(use_graph, event_reference):
    want, eventful = event_reference
    ro, X = rollout(load_graph("40"), use_graph=use_graph, **EVENT_KW)
    ro.enable_events(MASK, 1e-4, 0.6)
    ro.set_process_schedule(features=event_features())
    out = [ro.step_events()[1:] for _ in range(EVENT_STEPS)]
    if use_graph:
        assert ro._graph_ref is not None and ro._cap is not None   # (the segment graphs lived through the events in place)
    assert_same_event_state(event_state(ro, X, [e for e, _ in out], [w for _, w in out]), want, f"graph={use_graph}")


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [(5,), (2, 3), (3, 2)])
@pytest.mark.parametrize("use_graph", [False, True])
@torch.no_grad()
def test_run_events_with_a_schedule(use_graph, chunks, event_reference):
    """The step behind the eventful one is voided and run again: it must see its own row, not the one after; in chunks of
    3 + 2 the eventful third step is the last of its call (and in 2 + 3 the fifth, when it has events)."""
    want, eventful = event_reference
    ro, X = rollout(load_graph("40"), use_graph=use_graph, **EVENT_KW)
    ro.enable_events(MASK, 1e-4, 0.6)
    ro.set_process_schedule(features=event_features())
    launched, spec_launch = [], ro._spec_launch
    ro._spec_launch = lambda n: (launched.append(n), spec_launch(n))[1]
    ev, sw = [], []
    for n in chunks:
        e, w = ro.run_events(n)
        ev += e
        sw += w
    torch.cuda.synchronize()
    print(f"graph={use_graph} chunks={chunks}: blocks launched {launched}, eventful steps {eventful}")
    assert sum(launched) >= EVENT_STEPS and ro.steps_done == EVENT_STEPS
    if chunks == (5,):
        assert sum(launched) > EVENT_STEPS, launched   # at least one step was enqueued, voided and run again
    assert_same_event_state(event_state(ro, X, ev, sw), want, f"graph={use_graph} chunks={chunks}")
    assert int(ro._sched["home"]["flat"].item() if ro._sched["at"] is None else
               ro._sched["ring"][ro._sched["at"]]["flat"].item()) == EVENT_STEPS


@pytest.mark.gpu
@torch.no_grad()
def test_ensemble_events_with_a_schedule_per_trajectory():
    """Two perturbed trajectories, two schedules, events per trajectory: each equals its own event rollout after every step,
    and one that ends keeps the row of the step it ended in."""
    from test_ensemble_events import cfg1, rollout_of, union_rollout
    from graingraphnn_amd.topology import TopologyError
    steps = 5
    base = event_features()[0]
    feats = np.stack([np.stack([base * np.float32(1 + 1e-3 * r * (t + 1)) for t in range(2)]) for r in range(steps)])
    feats[:3, 0] = base   # (trajectory 0 keeps the fixture's rows for three steps)
    graphs = [cfg1("perturbed", 1000), cfg1("perturbed", 1001)]
    alone = []
    for t, g in enumerate(graphs):
        one, X1 = rollout_of(g, True, False)
        one.set_process_schedule(features=feats[:, t])
        seen, ended = [], None
        for _ in range(steps):
            try:
                one.step_events()
            except TopologyError:
                ended = one.steps_done
                break
            seen.append((X1["joint"].clone(), X1["grain"].clone(), {k: v.copy() for k, v in one.mask.items()}))
        alone.append((seen, ended, (X1["joint"].clone(), X1["grain"].clone())))
    ro, X, slices = union_rollout(graphs, True, False)
    off = {nt: [s[nt][0] for s in slices] + [slices[-1][nt][1]] for nt in ("grain", "joint")}
    ro.set_process_schedule(features=feats, traj_offsets=off)
    compared = 0
    for step in range(steps):
        ro.step_events()
        for t, st in enumerate(ro.trajectory_states()):
            seen, ended, final = alone[t]
            if ended is not None and step >= ended:
                assert st["ended_at"] == ended
                assert torch.equal(st["x_joint"], final[0]) and torch.equal(st["x_grain"], final[1]), (t, step)
                assert np.array_equal(st["x_joint"][0, 3:5].cpu().numpy(), feats[min(ended, steps - 1), t])
                continue
            xj, xg, mask = seen[step]
            assert st["ended_at"] is None
            assert torch.equal(st["x_joint"], xj) and torch.equal(st["x_grain"], xg), (t, step)
            assert np.array_equal(st["mask"]["grain"], mask["grain"]) and np.array_equal(st["mask"]["joint"], mask["joint"])
            assert np.array_equal(xj[0, 3:5].cpu().numpy(), feats[min(step + 1, steps - 1), t])
            compared += 1
    assert compared >= steps and sum(len(e) for e in ro.grain_events) > 0


QOI_KW = dict(patch_size=40.0, mesh_size=0.08, ini_height=2.0, final_height=50.0)


@pytest.mark.gpu
@torch.no_grad()
def test_qoi_beside_a_schedule():
    G, Rp = schedule_rows(12)
    a, _ = rollout(load_graph("40"), refresh_centres=True)
    a.enable_qoi(**QOI_KW)
    a.set_process_schedule(G, Rp)
    a.run(12)
    b, _ = rollout(load_graph("40"), refresh_centres=True)
    b.enable_qoi(**QOI_KW)
    for k in range(12):
        b.set_process_parameters(G[k], Rp[k])
        b.step()
    qa, qb = a.qoi(), b.qoi()
    assert qa["layers"] == qb["layers"] == 12 and torch.equal(qa["volume_traj"], qb["volume_traj"])
    assert torch.equal(qa["volume"], qb["volume"])


class _CountingLib:
    """The library with every call of an entry point noted."""

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


@pytest.mark.gpu
@pytest.mark.parametrize("plan", list(PLANS))
@torch.no_grad()
def test_off_means_off(plan):
    """Without a schedule a step makes the C-ABI calls it made before; with one, exactly one more, directly in front of the
    refresh; after clear_process_schedule() the old list again."""
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    ro, _ = rollout(load_graph("40"), plan, use_graph=False, refresh_centres=True)

    def counted_step():
        lib = be.lib
        be.lib = counting = _CountingLib(lib)
        try:
            ro.step()
        finally:
            be.lib = lib
        return counting.calls
    ro.step()
    before = counted_step()
    ro.set_process_schedule(*schedule_rows(4))
    ro.step()   # (the write of row 0 costs this step a rebuild of the edge records on the overlapped plan)
    with_schedule = counted_step()
    ro.clear_process_schedule()
    ro.step()
    after = counted_step()
    print(plan, "entry points per step:", len(before), before)
    assert "ggnn_process_schedule" not in before and before == after
    assert with_schedule.count("ggnn_process_schedule") == 1
    assert [c for c in with_schedule if c != "ggnn_process_schedule"] == before
    at = with_schedule.index("ggnn_process_schedule")
    assert with_schedule[at + 1].startswith("ggnn_step_refresh") and with_schedule[at - 1] == "ggnn_grain_centres"


@pytest.mark.gpu
@torch.no_grad()
def test_rollout_trajectories_with_schedules():
    from graingraphnn_amd.dist import rollout_trajectories
    steps = 5
    graphs = _perturbed(4)
    G, Rp = schedule_rows(steps, 4)
    R, Cm = product_models(31, 1.0, DEV)
    out = rollout_trajectories(R, Cm, graphs, 6, steps, 0, 1, DEV, schedule={"G": G.T, "R": Rp.T})
    assert set(out) == {"joint_xy", "grain_area_v"}
    table = np.stack([np.float32(1 - G / 10), np.float32(Rp / 2)], -1)
    feats = rollout_trajectories(R, Cm, graphs, 6, steps, 0, 1, DEV, schedule={"features": np.moveaxis(table, 0, 1)})
    for t, g in enumerate(graphs):
        one, X1 = rollout(g, "joint")
        one.set_process_schedule(G[:, t], Rp[:, t])
        one.run(steps)
        assert torch.equal(out["joint_xy"][t], X1["joint"][:, :2]) and torch.equal(out["grain_area_v"][t], X1["grain"][:, 3:5]), t
        assert torch.equal(feats["joint_xy"][t], out["joint_xy"][t])
    assert not torch.equal(out["joint_xy"][0], out["joint_xy"][1])
