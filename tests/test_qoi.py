"""Grain volumes and size statistics accumulated on the device during rollouts (GrainRollout.enable_qoi / qoi,
ggnn_qoi_accumulate / ggnn_qoi_finalize) against the float64 restatement of tests/qoicheck.py and the reference's own
numbers (tests/golden/make_golden_qoi.py: the cfg1 event trajectory, the 40 um no-flux trajectory, a static cfg1 run)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import qoicheck
from helpers import EDGE_TYPES, GOLDEN, load_graph, product_models, tt
from graingraphnn_amd import _lib, synthetic

DEV = "cuda"
GOLDENS = ("qoi_cfg1_events", "qoi_cfg1_static", "qoi_noflux_40_seed1")
BAR = 1e-4   # the project's parity bar: max|a - b| <= 1e-4 max|b|


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


# ---- the kernel's own problem: one union, no model ---------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 1025, 40, 1)   # grains per trajectory; trajectory 5 (40 grains) is entirely dead
DEAD_TRAJ = 5
LAYERS = 5
CONST = dict(patch_size=40.0, mesh_size=0.08, ini_height=2.0, final_height=50.0, frames=121, span=6, domain_factor=2.0)


def kernel_problem(order=None, seed=38):
    """Per trajectory (each from its own random stream, so that it is the same wherever it sits): layer 0 areas in
    [1e-4, 0.02], five layers of areas in [-1e-4, 0.02], excess volumes in [-2e-3, 2e-3]; about a fifth of the grains
    dead, more of them from layer 3 on.  `order`: the trajectories' order in the union."""
    order = list(range(len(SIZES))) if order is None else list(order)
    xs, ms = [], []
    for t in order:
        n, rs = SIZES[t], np.random.RandomState(seed + 17 * t)
        x = np.empty((LAYERS + 1, n, 2), np.float32)
        x[0, :, 0] = rs.uniform(1e-4, 0.02, n)
        x[1:, :, 0] = rs.uniform(-1e-4, 0.02, (LAYERS, n))
        x[:, :, 1] = rs.uniform(-2e-3, 2e-3, (LAYERS + 1, n))
        m = np.ones((LAYERS + 1, n), np.int32)
        if n > 1:
            m[:, rs.uniform(size=n) < 0.2] = 0
            m[3:, rs.uniform(size=n) < 0.1] = 0
        if t == DEAD_TRAJ:
            m[:] = 0
        xs.append(x)
        ms.append(m)
    off = np.concatenate([[0], np.cumsum([SIZES[t] for t in order])]).astype(np.int64)
    return np.concatenate(xs, 1), np.concatenate(ms, 1), off


def run_kernel(xg34, mask, off, capacity=LAYERS, guard=False, const=CONST):
    """The layers through backend.qoi_accumulate on one state, in place.  Returns a, T [L+1, N], the history
    [capacity + 1 (+ 1 guard row), N], A [L+1, n_traj], the flag word and the layer counter."""
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    L1, N = mask.shape
    xg = torch.zeros(N, 11, device=DEV)
    live = torch.empty(N, dtype=torch.int32, device=DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    st = {"a": torch.zeros(N, **f32), "T": torch.zeros(N, **f32), "e": torch.zeros(N, **f32),
          "layer": torch.full((1,), 77, dtype=torch.int32, device=DEV)}
    V0, words = torch.empty(N, **f32), torch.zeros(2, dtype=torch.int32, device=DEV)
    hist = torch.full((capacity + 1 + int(guard), N), -7.0, **f32)
    A = torch.empty(len(off) - 1, **f32)
    offs = torch.from_numpy(off).to(DEV)
    c = (const["domain_factor"], const["patch_size"] / const["mesh_size"] + 1,
         qoicheck.delta_h(const["span"], const["mesh_size"], const["ini_height"], const["final_height"], const["frames"]))
    a, T, As = [], [], []
    for k in range(L1):
        xg[:, 3:5] = torch.from_numpy(xg34[k]).to(DEV)
        live.copy_(torch.from_numpy(mask[k]).to(DEV))
        be.qoi_accumulate(xg, live, offs, c, st, st, V0, words[:1], words[1:], hist[:capacity + 1], capacity, A, init=k == 0)
        a.append(st["a"].cpu().numpy().copy())
        T.append(st["T"].cpu().numpy().copy())
        As.append(A.cpu().numpy().copy())
    return {"a": np.stack(a), "T": np.stack(T), "history": hist.cpu().numpy(), "A": np.stack(As), "flags": int(words[1]),
            "sync": int(words[0]), "layer": int(st["layer"]), "state": st, "V0": V0, "offsets": offs}


def kernel_reference(xg34, mask, off, variant=None):
    return qoicheck.restate(xg34, mask, offsets=off, variant=variant, **CONST)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_reference(name):
    """The float64 restatement on the recorded features gives the reference's area_traj, extraV_traj, volume_traj, d_mu and
    d_std to rtol 1e-12 and its histogram exactly."""
    d = golden(name)
    r = qoicheck.restate(d["xg34"], d["mask"], area0=d["area0"], **qoicheck.golden_kwargs(d))
    for k in ("area_traj", "extraV_traj", "volume_traj"):
        assert r[k].shape == d[k].shape == (int(d["steps"]) + 1, d["mask"].shape[1])
        np.testing.assert_allclose(r[k], d[k], rtol=1e-12, atol=0, err_msg=k)
    assert int(d["frames"]) == qoicheck.frames_default(float(d["ini_height"]), float(d["final_height"]))
    size, mu, std, counts, dens, edges = qoicheck.statistics(r["volume_traj"][-1], float(d["mesh_size"]))
    np.testing.assert_allclose(size, d["grain_size"], rtol=1e-12, atol=0)
    np.testing.assert_allclose([mu[0], std[0]], [d["d_mu"], d["d_std"]], rtol=1e-12, atol=0)
    assert np.array_equal(counts[0], d["hist_counts"]) and np.array_equal(edges[0], d["bin_edges"])
    np.testing.assert_allclose(dens[0], d["hist_density"], rtol=1e-12, atol=0)
    assert (d["mask"][-1] == 0).any() or name == "qoi_cfg1_static"   # eliminated grains are part of the statistics


@pytest.mark.parametrize("variant", qoicheck.VARIANTS)
def test_the_checks_reject_each_named_mistake(variant):
    """Both checks -- the element-wise bound of the kernel test on its problem (a union with dead grains, F = 2) and the
    parity bar on the goldens -- fail for every mistake qoicheck.restate can make on purpose."""
    x, m, off = kernel_problem()
    ref, bad = kernel_reference(x, m, off), kernel_reference(x, m, off, variant)
    worst = max(qoicheck.excess(bad["area_traj"], ref["area_traj"], np.abs(ref["area_traj"])),
                qoicheck.excess(bad["T"], ref["T"], ref["T_terms"]),
                qoicheck.excess(bad["volume_traj"], ref["volume_traj"], ref["volume_terms"]))
    assert worst > 10.0, (variant, worst)
    assert qoicheck.excess(ref["volume_traj"], ref["volume_traj"], ref["volume_terms"]) == 0.0
    # the goldens have F = 1, one trajectory and -- with the seeded weights the regressor's excess-volume output is zero at
    # every step -- e = 0: they cannot see those three mistakes, and see every other one
    d = golden("qoi_cfg1_events")
    bad = qoicheck.restate(d["xg34"], d["mask"], area0=d["area0"], variant=variant, **qoicheck.golden_kwargs(d))
    err = np.abs(bad["volume_traj"] - d["volume_traj"]).max() / np.abs(d["volume_traj"]).max()
    assert (err <= 1e-12) if variant in ("no_F", "one_union", "e_summed") else (err > 10 * BAR), (variant, err)


def test_finalize_problem_keeps_clear_of_the_bin_edges():
    """The histogram of the finalize test is compared exactly: on the float64 sizes no value lies within 1e-5 relative of
    a bin edge (seed chosen for it)."""
    x, m, off = kernel_problem()
    ref = kernel_reference(x, m, off)
    size = qoicheck.statistics(ref["volume_traj"][-1], CONST["mesh_size"], off)[0]
    assert (size[off[DEAD_TRAJ]:off[DEAD_TRAJ + 1]] == 0).all()
    size = size[size != 0]   # (the all-dead trajectory: exactly 0 = the first edge on both sides, test_accumulate_against_float64)
    for edges in (np.arange(0, 20, 1), np.arange(0, 20, 2)):
        gap = np.abs(size[:, None] - edges[None, :]) / np.maximum(np.abs(size[:, None]), 1e-300)
        assert gap.min() > 1e-5, gap.min()
    counts = qoicheck.statistics(ref["volume_traj"][-1], CONST["mesh_size"], off)[3]
    assert sum(int(c.sum()) for c in counts) > 1000   # (the sizes do fall into the bins)


def test_rollout_refuses_qoi_before_it_is_enabled():
    from graingraphnn_amd import GrainRollout
    assert GrainRollout.enable_qoi is not None
    ro = object.__new__(GrainRollout)
    ro._qoi = None
    with pytest.raises(_lib.GGNNError):
        ro.qoi()
    ro._enqueue_qoi()   # off: no launch, nothing touched (the object has no backend at all)


def test_entry_points_validate_on_the_host():
    """The ctypes mirror has the header's layout, and bad arguments are refused before anything would be launched."""
    import ctypes
    lib = _lib.load()
    assert ctypes.sizeof(_lib.QoiArgs) == 16 * 8 + 4 * 8 + 3 * 8 + 2 * 4
    assert lib.ggnn_qoi_accumulate(None, None) == -1
    assert lib.ggnn_qoi_accumulate(ctypes.byref(_lib.QoiArgs()), None) == -1
    buf = (ctypes.c_float * 32)()                 # (host memory: refused before a launch)
    p = ctypes.cast(buf, ctypes.c_void_p)
    A = _lib.QoiArgs(*([p] * 16), 11, 2, 1, 3, 0.5, 501.0, 30.0, 0, 0)
    assert lib.ggnn_qoi_accumulate(ctypes.byref(A), None) == -1        # domain_factor < 1
    A.domain_factor, A.ldx_grain = 1.0, 4
    assert lib.ggnn_qoi_accumulate(ctypes.byref(A), None) == -1        # no column 4
    assert lib.ggnn_qoi_finalize(None, None, None, 1, None, 1, 0.08, None, 0, None, None, None, None, None, None) == -1
    assert lib.ggnn_qoi_finalize(p, p, p, 2, p, 1, 0.08, p, 1026 + 1, p, p, p, p, p, None) == -1   # more edges than the kernel's bins
    assert lib.ggnn_qoi_finalize(p, p, p, 2, p, 1, 0.0, p, 3, p, p, p, p, p, None) == -1           # mesh_size


# ---- GPU: the kernels alone ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kernel_run():
    x, m, off = kernel_problem()
    return x, m, off, run_kernel(x, m, off), kernel_reference(x, m, off)


@pytest.mark.gpu
def test_accumulate_against_float64(kernel_run):
    """Every element of a, T and volume within 1e-5 of the sum of the absolute values of its terms: at most 2L + 1 fp32
    roundings of stored values, a sum and a normalisation carried in fp64 (< 4e-6)."""
    x, m, off, got, ref = kernel_run
    assert got["layer"] == LAYERS and got["flags"] == 0 and got["sync"] == 0
    worst = {"a": qoicheck.excess(got["a"], ref["area_traj"], np.abs(ref["area_traj"])),
             "T": qoicheck.excess(got["T"], ref["T"], ref["T_terms"]),
             "volume": qoicheck.excess(got["history"], ref["volume_traj"], ref["volume_terms"])}
    print("worst |got - ref| / (1e-5 sum|terms|):", worst)
    assert all(v <= 1.0 for v in worst.values()), worst
    lo, hi = off[DEAD_TRAJ], off[DEAD_TRAJ + 1]
    for k in ("a", "T", "history"):   # the all-dead trajectory: exact zeros (V0 of a_0 = 0 included), never a NaN
        assert np.isfinite(got[k]).all() and not got[k][:, lo:hi].any(), k
    assert (got["a"][m == 0] == 0).all()
    # A_k per trajectory
    live = m > 0
    for t in range(len(SIZES)):
        A = (x[:, off[t]:off[t + 1], 0].astype(np.float64) * live[:, off[t]:off[t + 1]]).sum(1) / CONST["domain_factor"] ** 2
        np.testing.assert_allclose(got["A"][:, t], A, rtol=2e-7, atol=0)


@pytest.mark.gpu
def test_accumulate_is_deterministic_and_position_independent(kernel_run):
    x, m, off, got, _ = kernel_run
    again = run_kernel(x, m, off)
    for k in ("a", "T", "history", "A"):
        assert np.array_equal(got[k], again[k]), k
    n = len(SIZES)
    for t in (3, 4):   # 65 grains (two waves, one block) and 1 025 grains (five blocks)
        lo, hi = off[t], off[t + 1]
        alone = run_kernel(x[:, lo:hi], m[:, lo:hi], np.array([0, hi - lo], np.int64))
        for k in ("a", "T", "history"):
            assert np.array_equal(alone[k], got[k][:, lo:hi]), (t, k)
        others = [u for u in range(n) if u != t]
        for pos in range(n):
            order = others[:pos] + [t] + others[pos:]
            xp, mp_, offp = kernel_problem(order)
            moved = run_kernel(xp, mp_, offp)
            for k in ("a", "T", "history"):
                assert np.array_equal(moved[k][:, offp[pos]:offp[pos + 1]], alone[k]), (t, pos, k)


@pytest.mark.gpu
def test_history_capacity_is_never_exceeded(kernel_run):
    """capacity = 3, five layers: rows 0..3 as in the full run, the guard row behind the history untouched, the overflow
    bit raised -- and GrainRollout.qoi() raises on it."""
    from graingraphnn_amd import GrainRollout
    x, m, off, full, _ = kernel_run
    got = run_kernel(x, m, off, capacity=3, guard=True)
    assert np.array_equal(got["history"][:4], full["history"][:4])
    assert (got["history"][4] == -7.0).all()
    assert got["flags"] & _lib.GGNN_FLAG_QOI_OVERFLOW and got["layer"] == LAYERS
    assert np.array_equal(got["a"], full["a"]) and np.array_equal(got["T"], full["T"])   # the accumulator goes on
    xg, ei, ea = load_graph("40")
    R, Cm = product_models(10020, 1.0, DEV)
    ro = GrainRollout(R, Cm, tt(xg, DEV), tt(ei, DEV), tt(ea, DEV), 6)
    ro.enable_qoi(40.0, 0.08, 2.0, 50.0, capacity=3)
    for _ in range(3):
        ro.step()
    assert ro.qoi()["layers"] == 3 and ro.qoi()["volume_traj"].shape == (4, 118)
    ro.step()
    ro.step()
    with pytest.raises(_lib.GGNNError):
        ro.qoi()


@pytest.mark.gpu
def test_finalize_against_numpy(kernel_run):
    from graingraphnn_amd.backend import default_backend
    x, m, off, got, _ = kernel_run
    be, st = default_backend(), got["state"]
    for step in (1, 2):
        edges = np.arange(0, 20, step)
        vol, size, mu, std, hist = be.qoi_finalize(got["V0"], st["T"], st["e"], got["offsets"], CONST["mesh_size"],
                                                   torch.from_numpy(edges.astype(np.float32)).to(DEV))
        v64 = vol.cpu().numpy().astype(np.float64)
        assert np.array_equal(vol.cpu().numpy(), got["history"][LAYERS])
        s64 = np.cbrt(6 * v64 / np.pi) * CONST["mesh_size"]
        np.testing.assert_allclose(size.cpu().numpy(), s64, rtol=2e-7, atol=0)
        for t in range(len(SIZES)):
            seg = s64[off[t]:off[t + 1]]
            assert abs(float(mu[t]) - seg.mean()) <= 1e-5 * abs(seg.mean()) + 1e-30, t
            assert abs(float(std[t]) - seg.std()) <= 1e-5 * seg.std() + 1e-30, t
            assert np.array_equal(hist[t].cpu().numpy(), np.histogram(seg, edges)[0]), t
    assert float(std[0]) == 0.0 and float(mu[DEAD_TRAJ]) == 0.0   # one grain; the all-dead trajectory


# ---- GPU: rollouts -------------------------------------------------------------------------------------------------------

def cfg1_rollout(d=None, events=False, **kw):
    from graingraphnn_amd import GrainRollout
    x, ei, ea = load_graph("40")
    R, Cm = product_models(10020, 1.0, DEV)
    X = tt(x, DEV)
    ro = GrainRollout(R, Cm, X, tt(ei, DEV), tt(ea, DEV), 6, **kw)
    if events:
        ro.enable_events({"grain": np.ones((118, 1)), "joint": np.ones((236, 1))}, 1e-4, 0.6)
    if d is not None:
        ro.enable_qoi(float(d["patch_size"]), float(d["mesh_size"]), float(d["ini_height"]), float(d["final_height"]),
                      area0=d["area0"], capacity=int(d["steps"]))
    return ro, X


def qoi_outputs(ro):
    q = ro.qoi()
    H = ro._qoi["home"]
    out = {k: q[k].cpu().numpy().copy() for k in ("volume", "size", "volume_traj")}
    out.update(T=H["T"].cpu().numpy().copy(), a=H["a"].cpu().numpy().copy(), e=H["e"].cpu().numpy().copy(),
               d_mu=q["d_mu"], d_std=q["d_std"], hist_counts=np.asarray(q["hist_counts"]), layers=q["layers"])
    return out


def assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (what, k)


def assert_golden(out, d, what):
    err = {"volume_traj": np.abs(out["volume_traj"] - d["volume_traj"]).max() / np.abs(d["volume_traj"]).max(),
           "d_mu": abs(out["d_mu"] - float(d["d_mu"])) / abs(float(d["d_mu"])),
           "d_std": abs(out["d_std"] - float(d["d_std"])) / abs(float(d["d_std"]))}
    print(what, "relative errors against the reference:", err)
    assert out["layers"] == int(d["steps"])
    assert all(np.isfinite(v) and v <= BAR for v in err.values()), (what, err)


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["joint", "overlapped"])
@torch.no_grad()
def test_graph_replay_equals_eager_steps(plan):
    """run(20) with hipGraphs (two replays of the 10-step graph; the layer counter lives on the device) = 20 eager step()s,
    bit for bit, and both within the kernel test's bound of the restatement on the eager loop's read-back states."""
    d = golden("qoi_cfg1_static")
    kw = dict(joint_launches=plan == "joint", concurrent=True)
    eager, Xe = cfg1_rollout(d, use_graph=False, **kw)
    states = [Xe["grain"][:, 3:5].cpu().numpy().copy()]
    for _ in range(20):
        eager.step()
        states.append(Xe["grain"][:, 3:5].cpu().numpy().copy())
    graphed, _ = cfg1_rollout(d, use_graph=True, **kw)
    assert graphed.RUN_UNROLL == 10
    graphed.run(20)
    a, b = qoi_outputs(eager), qoi_outputs(graphed)
    assert a["layers"] == 20
    assert_same_bits(a, b, plan)
    ref = qoicheck.restate(np.stack(states), np.ones((21, 118)), area0=d["area0"], **qoicheck.golden_kwargs(d))
    worst = {"T": qoicheck.excess(a["T"], ref["T"][-1], ref["T_terms"][-1]),
             "volume_traj": qoicheck.excess(a["volume_traj"], ref["volume_traj"], ref["volume_terms"])}
    print(plan, "worst |got - ref| / (1e-5 sum|terms|):", worst)
    assert all(v <= 1.0 for v in worst.values()), worst


def _decoder_plan_is(dec):
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    fused = bool(be.fused_decoder) and 236 >= be.fused_decoder_min_joints
    return fused == (dec == "fused")


@pytest.mark.gpu
@pytest.mark.parametrize("joint_launches", [True, False])
@torch.no_grad()
def test_static_golden(joint_launches):
    """20 static steps of cfg1: volume_traj, d_mu and d_std within the parity bar of the reference's."""
    d = golden("qoi_cfg1_static")
    ro, _ = cfg1_rollout(d, use_graph=True, joint_launches=joint_launches)
    ro.run(20)
    out = qoi_outputs(ro)
    assert_golden(out, d, f"static, joint_launches={joint_launches}, GGNN_DEC={os.environ.get('GGNN_DEC', 'auto')}")
    assert np.array_equal(out["hist_counts"], d["hist_counts"])


@pytest.mark.gpu
@pytest.mark.parametrize("dec", ["fused", "split"])
def test_static_golden_under_both_decoder_plans(dec):
    """The decoder plan is fixed per process (GGNN_DEC): the static golden, both launch plans, once more in a process of
    the plan this one does not run at this size."""
    if _decoder_plan_is(dec):
        return   # (test_static_golden ran under it here)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", __file__, "-k", "test_static_golden and not both"],
                       env=dict(os.environ, GGNN_DEC=dec), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "2 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.gpu
@torch.no_grad()
def test_event_golden_and_the_speculative_loop():
    """The reference's event trajectory (22, 75 and 27 eliminations in steps 3-5) through step_events(): the parity bar.
    run_events() -- whose eventful step 3 voids the steps enqueued behind it -- equals step_events() bit for bit on every
    QoI output."""
    d = golden("qoi_cfg1_events")
    steps = int(d["steps"])
    kw = dict(use_graph=True, refresh_centres=True, joint_launches=False, concurrent=True)
    a, _ = cfg1_rollout(d, events=True, **kw)
    for k in range(steps):
        a.step_events()
        assert np.array_equal(a.mask["grain"][:, 0], d["mask"][k + 1]), k
    out = qoi_outputs(a)
    assert_golden(out, d, "step_events")
    b, _ = cfg1_rollout(d, events=True, **kw)
    launched, launch = [], b._spec_launch
    b._spec_launch = lambda n: (launched.append(n), launch(n))[1]
    ev, _ = b.run_events(steps)
    assert [len(e) for e in ev] == [len(e) for e in a.grain_events]
    assert sum(launched) > steps, launched   # at least one step was enqueued, voided and run again
    assert_same_bits(out, qoi_outputs(b), "run_events")
    # in two calls, and mixed with step_events() on one rollout
    c, _ = cfg1_rollout(d, events=True, **kw)
    c.run_events(2)
    c.step_events()
    c.run_events(steps - 3)
    assert_same_bits(out, qoi_outputs(c), "run_events + step_events")


@pytest.mark.gpu
@torch.no_grad()
def test_noflux_golden():
    """noflux_40_seed1 (grain 0 is the boundary grain: area 0 after every boundary step) through step_events()."""
    from graingraphnn_amd import GrainRollout
    from test_noflux import fixture, initial_state
    d, f = golden("qoi_noflux_40_seed1"), fixture("noflux_40_seed1")
    R, Cm = product_models(int(f["weight_seed"]), 1.0, DEV)
    X, EI, EA, off, factor = initial_state(f, DEV)
    ro = GrainRollout(R, Cm, X, EI, EA, int(f["span"]), use_graph=True, refresh_centres=True, domain_factor=factor,
                      boundary="noflux", max_y=float(f["max_y"]))
    ro.enable_events({"grain": f["mask_grain"], "joint": f["mask_joint"]}, float(f["area_threshold"]), float(f["edge_threshold"]))
    ro.enable_qoi(float(d["patch_size"]), float(d["mesh_size"]), float(d["ini_height"]), float(d["final_height"]),
                  area0=d["area0"], capacity=int(d["steps"]))
    for k in range(int(d["steps"])):
        ro.step_events()
        assert np.array_equal(ro.mask["grain"][:, 0], d["mask"][k + 1]), k
    out = qoi_outputs(ro)
    assert_golden(out, d, "noflux")
    assert not out["a"][0] and not out["e"][0]


def _perturbed(n):
    x, ei, ea = load_graph("40")
    return [(synthetic.perturbed_copy(x, 1e-3, 1000 + t), ei, ea) for t in range(n)]


QOI_KW = dict(patch_size=40.0, mesh_size=0.08, ini_height=2.0, final_height=50.0)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank, world, port, out):
    import torch.distributed as dist
    from graingraphnn_amd.dist import rollout_trajectories
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    R, Cm = product_models(10020, 1.0, DEV)
    with torch.no_grad():
        res = rollout_trajectories(R, Cm, _perturbed(3), 6, 3, rank, world, DEV, qoi=QOI_KW)
    if rank == 0:
        torch.save({k: v.cpu() for k, v in res.items()}, out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@torch.no_grad()
def test_union_equals_the_individual_rollouts(tmp_path):
    """Three cfg1 trajectories perturbed as cfg4 does, as one disjoint-union rollout with traj_offsets = the three
    rollouts alone, bit for bit; through dist.rollout_trajectories(qoi=...) in one process and in a gloo world of two."""
    import torch.multiprocessing as mp
    from graingraphnn_amd import GrainRollout
    from graingraphnn_amd.dist import rollout_trajectories
    graphs = _perturbed(3)
    R, Cm = product_models(10020, 1.0, DEV)
    x, ei, ea, slices = synthetic.disjoint_union(graphs)
    X, EI, EA = synthetic.to_torch(x, ei, ea, DEV)
    ro = GrainRollout(R, Cm, X, EI, EA, 6, use_graph=True)
    ro.enable_qoi(traj_offsets=[0, 118, 236, 354], **QOI_KW)
    ro.run(3)
    u = ro.qoi()
    assert u["layers"] == 3 and len(u["hist"]) == 3 and u["d_mu"].shape == (3,)
    single = rollout_trajectories(R, Cm, graphs, 6, 3, 0, 1, DEV, qoi=QOI_KW)
    assert set(single) == {"joint_xy", "grain_area_v", "volume", "size"} and single["volume"].shape == (3, 118)
    for t in range(3):
        one = GrainRollout(R, Cm, tt(graphs[t][0], DEV), tt(graphs[t][1], DEV), tt(graphs[t][2], DEV), 6, use_graph=True)
        one.enable_qoi(**QOI_KW)
        one.run(3)
        q = one.qoi()
        lo, hi = slices[t]["grain"]
        assert torch.equal(q["volume_traj"], u["volume_traj"][:, lo:hi]), t
        assert torch.equal(q["volume"], u["volume"][lo:hi]) and torch.equal(q["size"], u["size"][lo:hi]), t
        assert q["d_mu"] == u["d_mu"][t] and q["d_std"] == u["d_std"][t], t
        assert np.array_equal(q["hist_counts"], u["hist_counts"][t]), t
        assert torch.equal(single["volume"][t], q["volume"]) and torch.equal(single["size"][t], q["size"]), t
    out = str(tmp_path / "gathered.pt")
    mp.spawn(_gloo_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = torch.load(out)
    for k, v in single.items():
        assert torch.equal(got[k], v.cpu()), k


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


# C-ABI calls of one eager step of the 40 um fixture with grain centres refreshed, as counted on the commit before the
# accumulator existed (the joint plan's ggnn_*_batch calls each cover both models)
STEP_CALLS = {"joint": 10, "overlapped": 12}


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["joint", "overlapped"])
@torch.no_grad()
def test_off_means_off(plan):
    """Without enable_qoi a step makes the launches it made before the feature (counted at the C ABI); with it, one more,
    and x and the predictions of run(10) are bit-equal: the accumulator only reads."""
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    kw = dict(joint_launches=plan == "joint", concurrent=True)
    d = golden("qoi_cfg1_static")
    calls = {}
    for on in (False, True):
        ro, _ = cfg1_rollout(d if on else None, use_graph=False, refresh_centres=True, **kw)
        ro.step()
        lib = be.lib
        be.lib = counting = _CountingLib(lib)
        try:
            ro.step()
        finally:
            be.lib = lib
        calls[on] = counting.calls
    assert "ggnn_qoi_accumulate" not in calls[False] and calls[True].count("ggnn_qoi_accumulate") == 1
    assert [c for c in calls[True] if c != "ggnn_qoi_accumulate"] == calls[False]
    print(plan, "entry points per step:", len(calls[False]), calls[False])
    assert len(calls[False]) == STEP_CALLS[plan]
    off, Xa = cfg1_rollout(None, use_graph=True, **kw)
    on, Xb = cfg1_rollout(d, use_graph=True, **kw)
    pa, pb = off.run(10), on.run(10)
    assert on.qoi()["layers"] == 10 and off._qoi is None
    for nt in Xa:
        assert torch.equal(Xa[nt], Xb[nt]), nt
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    assert sorted(off.state()) == ["grain_area_v", "joint_xy"]
