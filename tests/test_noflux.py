"""No-flux boundary condition (grain 0 wraps the domain; the reference's traj.BC == 'noflux'): masked CSR tables for
the forwards, the boundary step on the device, grain centres without min-image chaining, grain 0 kept out of the events,
and GrainRollout(boundary="noflux") on every launch plan against the reference's own trajectories
(tests/golden/make_golden_noflux.py: noflux_40_seed1.npz unfolded, noflux_80_seed3.npz folded by 2)."""
import os

import numpy as np
import pytest
import torch

from helpers import EDGE_TYPES, GOLDEN, assert_close, etk, product_models
from graingraphnn_amd import synthetic

GJ, JG, JJ = EDGE_TYPES
FIXTURES = ("noflux_40_seed1", "noflux_80_seed3")
DEV = "cuda"


def fixture(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def initial_state(d, device):
    """The reference loop's state before step 1: x and edge lengths after scale_feature_patchs (identity unfolded)."""
    x = {"grain": d["scaled_x_grain"], "joint": d["scaled_x_joint"]}
    ei = {et: d["ei_" + etk(et)] for et in EDGE_TYPES}
    ea = {et: d["scaled_ea_" + etk(et)].reshape(-1, 1) for et in EDGE_TYPES}
    tt = lambda v, dt=None: torch.from_numpy(np.array(v, copy=True, order="C")).to(device)
    return ({k: tt(v) for k, v in x.items()}, {k: tt(v) for k, v in ei.items()}, {k: tt(v) for k, v in ea.items()},
            tt(d["domain_offset"]), float(d["domain_factor"]))


# ---- CPU -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_a_noflux_structure(name):
    """Grain 0 is the boundary grain: its junctions lie on the walls, and after the boundary step every junction is in
    [0,1] x [0,max_y] in the global frame."""
    d = fixture(name)
    jg = d["ei_" + etk(JG)]
    walls = np.unique(jg[0, jg[1] == 0])
    assert len(walls) >= 30
    f, off, max_y = float(d["domain_factor"]), d["domain_offset"], float(d["max_y"])
    xy = (d["s1_bnd_x_joint"][:, :2] + off) / np.float32(f)
    assert (xy >= 0).all() and (xy[:, 0] <= 1).all() and (xy[:, 1] <= max_y).all()
    b = xy[walls]
    on_wall = (b[:, 0] == 0) | (b[:, 0] == 1) | (b[:, 1] == 0) | (b[:, 1] == max_y)
    assert on_wall.all()
    # the forwards' lists lose exactly grain 0's edges
    assert d["s1_fwd_ei_" + etk(GJ)].shape[1] == d["ei_" + etk(GJ)].shape[1] - int((d["ei_" + etk(GJ)][0] == 0).sum())


@pytest.mark.parametrize("name", FIXTURES)
def test_noflux_forward_edges_matches_the_reference(name):
    d = fixture(name)
    ei = {et: torch.from_numpy(d["ei_" + etk(et)]) for et in EDGE_TYPES}
    ea = {et: torch.from_numpy(d["ea_" + etk(et)]).view(-1, 1) for et in EDGE_TYPES}
    fei, fea = synthetic.noflux_forward_edges(ei, ea)
    for et in EDGE_TYPES:
        ref = d["s1_fwd_ei_" + etk(et)]
        assert np.array_equal(fei[et].numpy(), ref), et
        keep = ei[et][0 if et[0] == "grain" else 1] > 0 if "grain" in (et[0], et[-1]) else torch.ones(ref.shape[1], dtype=bool)
        assert torch.equal(fea[et], ea[et][keep])


def test_scale_feature_patchs_noflux_matches_the_reference():
    d = fixture("noflux_80_seed3")
    x = {"grain": d["x_grain"].copy(), "joint": d["x_joint"].copy()}
    ea = {et: d["ea_" + etk(et)].copy() for et in EDGE_TYPES}
    off = synthetic.scale_feature_patchs(float(d["domain_factor"]), x, ea, boundary="noflux")
    assert np.array_equal(off, d["domain_offset"])
    assert np.array_equal(x["grain"], d["scaled_x_grain"]) and np.array_equal(x["joint"], d["scaled_x_joint"])
    for et in EDGE_TYPES:
        assert np.array_equal(ea[et].reshape(-1), d["scaled_ea_" + etk(et)])
    with pytest.raises(ValueError):
        synthetic.scale_feature_patchs(2.0, x, ea, boundary="open")


def test_rollout_refuses_an_unknown_boundary():
    from graingraphnn_amd import GrainRollout, _lib
    with pytest.raises(_lib.GGNNError):
        GrainRollout(None, None, {}, {}, {}, 6, boundary="open")


# ---- GPU: masked CSR ------------------------------------------------------------------------------------------------

def _host_filtered(ei, skip_src, skip_dst):
    keep = np.flatnonzero((ei[0] != skip_src) & (ei[1] != skip_dst))
    return ei[:, keep], keep


def _check_masked(be, csr, ei_full, n_src, n_dst, skip_src, skip_dst):
    sub, keep = _host_filtered(ei_full, skip_src, skip_dst)
    ref = be.build_csr(torch.from_numpy(np.ascontiguousarray(sub)).to(DEV), n_src, n_dst)
    k = sub.shape[1]
    assert int(csr.E_dev.item()) == k
    assert torch.equal(csr.rowptr, ref.rowptr)
    assert torch.equal(csr.col[:k], ref.col[:k])
    assert torch.equal(csr.row[:k], ref.row[:k])
    assert np.array_equal(csr.perm[:k].cpu().numpy(), keep[ref.perm[:k].cpu().numpy()])   # ids of the FULL list
    nu = int(ref.unit_ptr[-1])
    assert torch.equal(csr.unit_ptr, ref.unit_ptr) and torch.equal(csr.units[:nu], ref.units[:nu])
    assert bool((csr.col[k:] == 0).all()) and bool((csr.perm[k:] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_masked_csr_equals_the_csr_of_the_filtered_list(name):
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    d = fixture(name)
    ng, nj = d["x_grain"].shape[0], d["x_joint"].shape[0]
    gj, jg = np.ascontiguousarray(d["ei_" + etk(GJ)]), np.ascontiguousarray(d["ei_" + etk(JG)])
    lists = [(torch.from_numpy(gj).to(DEV), ng, nj), (torch.from_numpy(jg).to(DEV), nj, ng), (torch.from_numpy(jg).to(DEV), nj, ng)]
    built = be.build_csr_batch(lists, masks=[(0, -1), (-1, 0), (-1, -1)])
    _check_masked(be, built[0], gj, ng, nj, 0, -1)
    _check_masked(be, built[1], jg, nj, ng, -1, 0)
    plain = be.build_csr(lists[2][0], nj, ng)   # skip = -1: the unmasked tables
    assert built[2].E_dev is None
    for a in ("rowptr", "col", "perm", "row", "unit_ptr", "units"):
        assert torch.equal(getattr(built[2], a), getattr(plain, a)), a
    # the in-place refill of the event loop: tables of the initial size, refilled with the lists after an event
    ip = be.csr_in_place([(gj.shape[1], ng, nj), (jg.shape[1], nj, ng)], DEV, [(0, -1), (-1, 0)])
    ip.rebuild([lists[0][0], lists[1][0]])
    step = next(s for s in range(1, int(d["steps"]) + 1) if d[f"s{s}_ei_" + etk(JG)].shape[1] < jg.shape[1])
    gj2, jg2 = np.ascontiguousarray(d[f"s{step}_ei_" + etk(GJ)]), np.ascontiguousarray(d[f"s{step}_ei_" + etk(JG)])
    got = ip.rebuild([torch.from_numpy(gj2).to(DEV), torch.from_numpy(jg2).to(DEV)])
    _check_masked(be, got[0], gj2, ng, nj, 0, -1)
    _check_masked(be, got[1], jg2, nj, ng, -1, 0)


# ---- GPU: boundary step -----------------------------------------------------------------------------------------------

def _boundary_reference(xj, xg, ei_gj, off, f, max_y):
    """torch restatement of test.py:446-463 (fp32, CPU)."""
    xg[0, :2] = 0.5
    xg[0, 3:5] = 0
    xg[0, -1] = 0
    xj[:, :2] = (xj[:, :2] + off) / f
    for p in ei_gj[1, (ei_gj[0] == 0).nonzero().view(-1)]:
        dist = torch.stack([xj[p, 0], 1 - xj[p, 0], xj[p, 1], max_y - xj[p, 1]])
        k = int(dist.argmin())
        if k == 0:
            xj[p, 0] = 0
        elif k == 1:
            xj[p, 0] = 1
        elif k == 2:
            xj[p, 1] = 0
        else:
            xj[p, 1] = max_y
    xj[:, 0] = torch.clamp(xj[:, 0], min=0, max=1)
    xj[:, 1] = torch.clamp(xj[:, 1], min=0, max=max_y)
    xj[:, :2] = xj[:, :2] * f - off


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_boundary_step_is_bit_equal_to_the_reference_formulation(name):
    from graingraphnn_amd.backend import default_backend
    from graingraphnn_amd.engine import GraphCSR
    be = default_backend()
    d = fixture(name)
    X, EI, _, off, f = initial_state(d, "cpu")
    rs = np.random.RandomState(7)
    # move the junctions by up to a few percent of the domain so that some leave it, and place one wall junction exactly
    # as far from two walls (x = y = 0.25 in the global frame: the first minimum, x = 0, wins)
    X["joint"][:, :2] += torch.from_numpy(rs.uniform(-0.03, 0.03, (X["joint"].shape[0], 2)).astype(np.float32)) * f
    p = int(EI[GJ][1, EI[GJ][0] == 0][0])
    X["joint"][p, :2] = torch.tensor([0.25, 0.25]) * f - off[p]
    ref_j, ref_g = X["joint"].clone(), X["grain"].clone()
    _boundary_reference(ref_j, ref_g, EI[GJ], off if f > 1 else 0, f, 1.0)
    assert float(((ref_j[p, :2] + off[p]) / f)[0]) == 0.0
    xj, xg = X["joint"].to(DEV), X["grain"].to(DEV)
    g = GraphCSR(be, {et: EI[et].to(DEV) for et in EDGE_TYPES}, {"grain": xg.size(0), "joint": xj.size(0)}, boundary="noflux")
    before = torch.empty(xj.size(0), 2, device=DEV)
    be.noflux_boundary(g.csr_full[JG], xj, xg, f, off.to(DEV) if f > 1 else None, 1.0, joints_before=before)
    assert torch.equal(before.cpu(), X["joint"][:, :2])
    assert torch.equal(xj.cpu(), ref_j)
    assert torch.equal(xg.cpu(), ref_g)


# ---- GPU: forwards and rollouts -------------------------------------------------------------------------------------

def _rollout(d, plan="overlapped", use_graph=False):
    from graingraphnn_amd import GrainRollout
    R, Cm = product_models(int(d["weight_seed"]), 1.0, DEV)
    X, EI, EA, off, f = initial_state(d, DEV)
    kw = dict(joint_launches=plan == "joint", concurrent=plan != "single")
    ro = GrainRollout(R, Cm, X, EI, EA, int(d["span"]), use_graph=use_graph, refresh_centres=True, domain_factor=f,
                      domain_offset=off if f > 1 else None, boundary="noflux", max_y=float(d["max_y"]), **kw)
    return ro, X


def _check_state(ro, X, d, step, what):
    live_j = torch.from_numpy(d[f"s{step}_mask_joint"][:, 0] > 0).to(DEV)
    live_g = torch.from_numpy(d[f"s{step}_mask_grain"][:, 0] > 0).to(DEV)
    assert_close(X["joint"][live_j], d[f"s{step}_x_joint"][live_j.cpu().numpy()], f"{what}: step {step} junctions")
    assert_close(X["grain"][live_g], d[f"s{step}_x_grain"][live_g.cpu().numpy()], f"{what}: step {step} grains")


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
@torch.no_grad()
def test_forwards_on_the_masked_graph_match_the_reference(name):
    d = fixture(name)
    ro, X = _rollout(d, plan="joint")
    pred = ro.step()
    for k in ("joint", "grain", "grain_area", "edge_event", "edge"):
        assert_close(pred[k], d["s1_pred_" + k], f"{name} step 1 {k}")
    _check_state(ro, X, d, 1, name)
    ea = ro.edge_attr_dict()
    for et in EDGE_TYPES:   # the full lists' lengths, grain 0's edges included (test.py:562-575)
        assert_close(ea[et].view(-1), d["s1_ea_" + etk(et)], f"{name} step 1 lengths {et}")


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["joint", "single", "overlapped"])
@pytest.mark.parametrize("use_graph", [False, True])
@torch.no_grad()
def test_static_rollout_matches_the_quiet_steps(plan, use_graph):
    """80 um folded fixture: steps 1-2 are quiet in the reference; step() then run() on every launch plan."""
    d = fixture("noflux_80_seed3")
    assert all(len(d[f"s{s}_grain_event"]) == 0 and len(d[f"s{s}_switching_list"]) == 0 for s in (1, 2))
    ro, X = _rollout(d, plan, use_graph)
    ro.step()
    _check_state(ro, X, d, 1, f"{plan} step()")
    ro2, X2 = _rollout(d, plan, use_graph)
    ro2.RUN_UNROLL = 2
    ro2.run(2)
    _check_state(ro2, X2, d, 2, f"{plan} run()")


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("mode", ["step_events", "run_events"])
@pytest.mark.parametrize("use_graph", [False, True])
@torch.no_grad()
def test_event_rollout_reproduces_the_noflux_trajectory(name, mode, use_graph):
    d = fixture(name)
    ro, X = _rollout(d, "overlapped", use_graph)
    ro.enable_events({"grain": d["mask_grain"], "joint": d["mask_joint"]}, float(d["area_threshold"]),
                     float(d["edge_threshold"]))
    steps = int(d["steps"])
    if mode == "run_events":
        ev, sw = ro.run_events(steps)
    else:
        ev, sw = [], []
        for step in range(1, steps + 1):
            _, e, s = ro.step_events()
            ev.append(e)
            sw.append(s)
            assert sorted(e.tolist()) == sorted(d[f"s{step}_grain_event"].tolist()), step
            for et in EDGE_TYPES:
                assert np.array_equal(ro.edge_index[et].cpu().numpy(), d[f"s{step}_ei_" + etk(et)]), (step, et)
            _check_state(ro, X, d, step, name)
    assert sum(len(e) for e in ev) > 0 and sum(len(s) for s in sw) > 0
    for step in range(1, steps + 1):
        assert sorted(ev[step - 1].tolist()) == sorted(d[f"s{step}_grain_event"].tolist()), step
        assert len(sw[step - 1]) == len(d[f"s{step}_switching_list"]), step
    for et in EDGE_TYPES:
        assert np.array_equal(ro.edge_index[et].cpu().numpy(), d[f"s{steps}_ei_" + etk(et)]), et
    assert np.array_equal(ro.mask["grain"], d[f"s{steps}_mask_grain"])
    assert np.array_equal(ro.mask["joint"], d[f"s{steps}_mask_joint"])
    _check_state(ro, X, d, steps, f"{name} {mode}")
    ea = ro.edge_attr_dict()
    for et in EDGE_TYPES:
        assert_close(ea[et].view(-1), d[f"s{steps}_ea_" + etk(et)], f"{name} lengths {et}")


@pytest.mark.gpu
@torch.no_grad()
def test_boundary_grain_never_makes_a_step_eventful():
    """40 um fixture, step 1: the regressor puts grain 0's area (-1.15e-3) below every interior grain's (>= -1.11e-3).
    With the threshold between them only grain 0 is below it -- and it is not a candidate (test.py:421-422): no eventful
    step, neither in the device-side count nor on the host."""
    from graingraphnn_amd.backend import default_backend
    d = fixture("noflux_40_seed1")
    area = torch.from_numpy(d["s1_pred_grain_area"])
    thr = float((area[0] + area[1:].min()) / 2)
    assert float(area[0]) < thr < float(area[1:].min())
    for mode in ("step_events", "run_events"):
        ro, X = _rollout(d)
        ro.enable_events({"grain": d["mask_grain"], "joint": d["mask_joint"]}, thr, 0.99)
        if mode == "run_events":
            ev, sw = ro.run_events(1)
        else:
            _, e, s = ro.step_events()
            ev, sw = [e], [s]
        assert len(ev[0]) == 0 and len(sw[0]) == 0
        # the device-side count: grain 0 alone would fire without the exclusion
        be, p = default_backend(), ro.pred
        flags = torch.zeros(2, dtype=torch.int32, device=DEV)
        ei = ro.edge_index[JJ]
        be.detect_events(p["grain_area"], ro._live_grain, thr, p["edge_event"], ei, 10.0, flags)
        with_grain0 = int(flags[0])
        be.detect_events(p["grain_area"], ro._live_grain, thr, p["edge_event"], ei, 10.0, flags, skip_grain=0)
        assert int(flags[0]) == with_grain0 - 1 and int(ro._live_grain[0]) == 1
    assert with_grain0 >= 1
