"""No-flux ensembles: a disjoint union of no-flux trajectories, every one with a boundary grain of its own (its
local grain 0).  The masked CSR tables of a union (ggnn_build_csr_batch_traj), the boundary step per trajectory
(ggnn_noflux_boundary_traj), the grain centres on a union, topology.EnsembleSessions.apply(skip_local_grain=0), and
GrainRollout(boundary="noflux", traj_offsets=...) / dist.rollout_trajectories(boundary="noflux") against the trajectories'
own rollouts, bit for bit, and against the reference's recorded no-flux trajectories."""
import numpy as np
import pytest
import torch

from helpers import EDGE_TYPES, etk, product_models, tt
from graingraphnn_amd import _lib, synthetic
from graingraphnn_amd.topology import EnsembleSessions, TopologySession, check_noflux_union, check_traj_offsets
from test_ensemble_events import (QOI_KW, _CountingLib, assert_same_state, check_union_against_own_rollouts, qoi_rows,
                                  snapshot)
from test_noflux import _boundary_reference, _check_state, fixture

GJ, JG, JJ = EDGE_TYPES
DEV = "cuda"
F40, F80 = "noflux_40_seed1", "noflux_80_seed3"


def nf_graph(d, seed=None, sigma=0.0):
    """A fixture's state before step 1 as a trajectory (x, ei, ea); `seed`: with its junctions moved (synthetic.perturbed_copy)."""
    x = {"grain": d["scaled_x_grain"].copy(), "joint": d["scaled_x_joint"].copy()}
    if seed is not None:
        x = synthetic.perturbed_copy(x, sigma, seed)
    ei = {et: d["ei_" + etk(et)].copy() for et in EDGE_TYPES}
    ea = {et: d["scaled_ea_" + etk(et)].reshape(-1, 1).copy() for et in EDGE_TYPES}
    return x, ei, ea


def offsets_of(slices):
    return {nt: [s[nt][0] for s in slices] + [slices[-1][nt][1]] for nt in ("grain", "joint")}


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def _update_inputs(d, step):
    """What the reference's Cmodel.update saw at `step` of the 40 um fixture: the lists and masks of the step before, the
    junctions after Rmodel.update (models.py:503-510, fp32) and the step's predictions."""
    prev = lambda key: d[key] if step == 1 else d[f"s{step - 1}_" + key]
    xj = (d["scaled_x_joint"] if step == 1 else d[f"s{step - 1}_x_joint"]).copy()
    yj = d[f"s{step}_pred_joint"].copy()
    xj[:, :2] += yj / np.float32(5.0)
    xj[:, 6:8] = yj
    prob = torch.sigmoid(torch.from_numpy(d[f"s{step}_pred_edge_event"])).numpy()
    return dict(xj=np.ascontiguousarray(xj), yj=yj, yg=d[f"s{step}_pred_grain"].copy(), area=d[f"s{step}_pred_grain_area"].copy(),
                prob=prob, mg=prev("mask_grain").astype(np.int64).copy(), mj=prev("mask_joint").astype(np.int64).copy(),
                pp=prev("ei_" + etk(JJ)).copy(), pq=prev("ei_" + etk(JG)).copy())


def test_ensemble_apply_skips_every_trajectorys_boundary_grain():
    """Steps 3, 4 and 5 of the 40 um fixture (eliminations, a switch) as three trajectories of one union, every boundary
    grain's predicted area forced below the threshold: apply(skip_local_grain=0) gives every trajectory what its own
    TopologySession gives with the candidates of the single rollout (test.py:418-422), bit for bit, and no boundary grain
    is ever an event; without the keyword the boundary grains are candidates."""
    d = fixture(F40)
    thr, edge_thr = float(d["area_threshold"]), float(d["edge_threshold"])
    parts = [_update_inputs(d, s) for s in (3, 4, 5)]
    for p in parts:
        p["area"][0] = -1.0
    from test_ensemble_events import union_of
    u, off_g, off_j = union_of(parts)
    assert check_noflux_union(off_g, off_j).tolist() == off_g[:-1].tolist()
    ens = EnsembleSessions(u["pp"], u["pq"], off_g, off_j)
    res = ens.apply(u["xj"], u["yj"], u["yg"][:, 0], u["prob"], u["area"], u["mg"], u["mj"], np.ones((3, 2), np.int32), None,
                    thr, edge_thr, skip_local_grain=0)
    assert not res["refused"] and res["changed"] == [0, 1, 2]
    assert not np.isin(off_g[:-1], res["events"]).any(), "a boundary grain was eliminated"
    assert (u["mg"][off_g[:-1], 0] == 1).all()
    pp = res["lists"][:2 * res["n_pp"]].reshape(2, -1)
    pq = res["lists"][2 * res["n_pp"]:2 * (res["n_pp"] + res["n_pq"])].reshape(2, -1)
    seg_pp, seg_pq = ens.segments()
    n_events = 0
    for t, p in enumerate(parts):
        own = {k: v.copy() for k, v in p.items()}
        ses = TopologySession(own["pp"], own["pq"], own["mj"].shape[0], own["mg"].shape[0])
        ge = np.flatnonzero((own["mg"][:, 0] > 0) & (own["area"] < np.float32(thr)))
        ge = ge[np.argsort(own["area"][ge], kind="stable")]
        assert ge[0] == 0, "the boundary grain is the smallest candidate: the exclusion is what keeps it out"
        ev, sw = ses.apply(own["xj"], own["yj"], own["yg"][:, 0], own["prob"], ge[ge != 0], own["mg"], own["mj"], edge_thr)
        own_pp, own_pq, _ = ses.export()
        g0, g1, j0, j1 = off_g[t], off_g[t + 1], off_j[t], off_j[t + 1]
        got_ev, got_sw = res["per_traj"][t]
        assert np.array_equal(got_ev, ev) and np.array_equal(got_sw, sw), t
        assert np.array_equal(u["xj"][j0:j1], own["xj"]) and np.array_equal(u["yj"][j0:j1], own["yj"]), t
        assert np.array_equal(u["mg"][g0:g1], own["mg"]) and np.array_equal(u["mj"][j0:j1], own["mj"]), t
        assert np.array_equal(pp[:, seg_pp[t]:seg_pp[t + 1]] - j0, own_pp), t
        assert np.array_equal(pq[:, seg_pq[t]:seg_pq[t + 1]] - np.array([[j0], [g0]]), own_pq), t
        n_events += len(ev)
    assert n_events >= 3
    # without the keyword the boundary grains are candidates like any other grain
    u2, _, _ = union_of([dict(p, area=p["area"].copy()) for p in (_update_inputs(d, s) for s in (3, 4, 5))])
    u2["area"][off_g[:-1]] = -1.0
    ens2 = EnsembleSessions(u2["pp"], u2["pq"], off_g, off_j)
    res2 = ens2.apply(u2["xj"], u2["yj"], u2["yg"][:, 0], u2["prob"], u2["area"], u2["mg"], u2["mj"], np.ones((3, 2), np.int32),
                      None, thr, edge_thr)
    assert len(res2["refused"]) + int(np.isin(off_g[:-1], res2["events"]).sum()) == 3


def test_constructor_and_offset_validation():
    """What is refused before any device work: a trajectory with junctions and no grain, offsets on a periodic rollout,
    and enable_* offsets that are not the constructor's."""
    from graingraphnn_amd import GrainRollout
    from graingraphnn_amd.rollout import resolve_traj_offsets
    x = {"grain": torch.zeros(6, 11), "joint": torch.zeros(12, 8)}
    ok = {"grain": [0, 3, 3, 6], "joint": [0, 6, 6, 12]}   # (an empty trajectory in the middle is allowed)
    og, oj = check_traj_offsets(ok, 6, 12)
    assert check_noflux_union(og, oj).tolist() == [0, 3]
    with pytest.raises(_lib.GGNNError, match="at least one grain"):   # trajectory 1: junctions, no grain
        GrainRollout(None, None, x, {}, {}, 6, boundary="noflux", traj_offsets={"grain": [0, 3, 3, 6], "joint": [0, 4, 8, 12]})
    with pytest.raises(_lib.GGNNError, match="at least one grain"):   # ... and grains without a junction
        check_noflux_union(*check_traj_offsets({"grain": [0, 2, 4, 6], "joint": [0, 6, 6, 12]}, 6, 12))
    with pytest.raises(_lib.GGNNError, match="traj_offsets"):         # not offsets at all
        GrainRollout(None, None, x, {}, {}, 6, boundary="noflux", traj_offsets={"grain": [0, 3, 7], "joint": [0, 6, 12]})
    with pytest.raises(_lib.GGNNError, match="noflux"):               # a periodic union passes them to enable_events
        GrainRollout(None, None, x, {}, {}, 6, boundary="periodic", traj_offsets=ok)
    own = (og, oj)
    assert resolve_traj_offsets(own, None, "enable_events") is own
    assert resolve_traj_offsets(own, ok, "enable_events") is own
    assert resolve_traj_offsets(own, ok["grain"], "enable_qoi") is own
    assert resolve_traj_offsets(None, None, "enable_events") is None
    for bad in ({"grain": [0, 3, 6], "joint": [0, 6, 12]}, {"grain": ok["grain"]}, {"grain": ok["grain"], "joint": [0, 6, 7, 12]}):
        with pytest.raises(_lib.GGNNError, match="differ"):
            resolve_traj_offsets(own, bad, "enable_events")
    with pytest.raises(_lib.GGNNError, match="differ"):
        resolve_traj_offsets(own, [0, 3, 6], "enable_qoi")
    with pytest.raises(_lib.GGNNError, match="noflux.*construct"):     # no constructor offsets: says where they go
        resolve_traj_offsets(None, ok, "enable_events")


# ---- GPU: masked tables of a union --------------------------------------------------------------------------------------------

def _union_lists(parts):
    """[(gj [2, E], jg [2, E], n_grain, n_joint) or None = an empty trajectory] -> (gj, jg, grain offsets, junction offsets)."""
    og, oj, gjs, jgs = [0], [0], [], []
    for p in parts:
        if p is not None:
            gjs.append(p[0] + np.array([[og[-1]], [oj[-1]]]))
            jgs.append(p[1] + np.array([[oj[-1]], [og[-1]]]))
        og.append(og[-1] + (0 if p is None else p[2]))
        oj.append(oj[-1] + (0 if p is None else p[3]))
    cat = lambda v: np.ascontiguousarray(np.concatenate(v, axis=1).astype(np.int64))
    return cat(gjs), cat(jgs), np.asarray(og, np.int64), np.asarray(oj, np.int64)


def _check_masked_union(be, csr, ei_full, n_src, n_dst, boundary_grains, side):
    """test_noflux._check_masked for a union: the tables equal those of the list without every edge whose grain (row `side`
    of the list) is a boundary grain; perm counts in the FULL list; E_kept = the kept count."""
    keep = np.flatnonzero(~np.isin(ei_full[side], boundary_grains))
    sub = ei_full[:, keep]
    ref = be.build_csr(torch.from_numpy(np.ascontiguousarray(sub)).to(DEV), n_src, n_dst)
    k = sub.shape[1]
    assert 0 < k < ei_full.shape[1]
    assert int(csr.E_dev.item()) == k
    assert torch.equal(csr.rowptr, ref.rowptr)
    assert torch.equal(csr.col[:k], ref.col[:k]) and torch.equal(csr.row[:k], ref.row[:k])
    assert np.array_equal(csr.perm[:k].cpu().numpy(), keep[ref.perm[:k].cpu().numpy()])
    nu = int(ref.unit_ptr[-1])
    assert torch.equal(csr.unit_ptr, ref.unit_ptr) and torch.equal(csr.units[:nu], ref.units[:nu])
    assert bool((csr.col[k:] == 0).all()) and bool((csr.perm[k:] == 0).all())


@pytest.mark.gpu
def test_masked_union_tables_equal_the_tables_of_the_filtered_lists():
    """[40 um, an EMPTY trajectory, the 80 um lists, 40 um]: a fresh build and the in-place refill after a list shrank."""
    from graingraphnn_amd.backend import default_backend
    from graingraphnn_amd.engine import NOFLUX_MASKS, noflux_unions
    be = default_backend()
    d40, d80 = fixture(F40), fixture(F80)
    part = lambda d, pre="": (d[pre + "ei_" + etk(GJ)], d[pre + "ei_" + etk(JG)], d["x_grain"].shape[0], d["x_joint"].shape[0])
    gj, jg, og, oj = _union_lists([part(d40), None, part(d80), part(d40)])
    assert og.tolist() == [0, 101, 101, 501, 602] and oj.tolist() == [0, 198, 198, 996, 1194]
    bnd = check_noflux_union(og, oj)
    assert bnd.tolist() == [0, 101, 501]
    ng, nj = int(og[-1]), int(oj[-1])
    og_dev = torch.from_numpy(og).to(DEV)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    masks, unions = [NOFLUX_MASKS[GJ], NOFLUX_MASKS[JG], None], noflux_unions(og_dev)[:2] + [None]
    built = be.build_csr_batch([(dev(gj), ng, nj), (dev(jg), nj, ng), (dev(jg), nj, ng)], masks=masks, unions=unions)
    _check_masked_union(be, built[0], gj, ng, nj, bnd, 0)
    _check_masked_union(be, built[1], jg, nj, ng, bnd, 1)
    plain = be.build_csr(dev(jg), nj, ng)
    assert built[2].E_dev is None
    for a in ("rowptr", "col", "perm", "row", "unit_ptr", "units"):
        assert torch.equal(getattr(built[2], a), getattr(plain, a)), a
    # global skips on the same lists leave out grain 0's edges alone: the union's tables differ from them
    alone = be.build_csr_batch([(dev(gj), ng, nj)], masks=[(0, -1)])[0]
    assert int(alone.E_dev.item()) > int(built[0].E_dev.item())
    # the event loop's refill: the first trajectory's lists after its step 4 (eliminations), the others as they were
    ip = be.csr_in_place([(gj.shape[1], ng, nj), (jg.shape[1], nj, ng)], DEV, masks[:2], unions=unions[:2])
    first = ip.rebuild([dev(gj), dev(jg)])
    _check_masked_union(be, first[0], gj, ng, nj, bnd, 0)
    gj2, jg2, og2, _ = _union_lists([part(d40, "s4_"), None, part(d80), part(d40)])
    assert gj2.shape[1] < gj.shape[1] and np.array_equal(og2, og)
    got = ip.rebuild([dev(gj2), dev(jg2)])
    _check_masked_union(be, got[0], gj2, ng, nj, bnd, 0)
    _check_masked_union(be, got[1], jg2, nj, ng, bnd, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [[3], [0, 2, 0, 1, 3, 0], [2, 1, 0, 0, 2]])
def test_masked_union_tables_at_the_edges_of_the_offsets(sizes):
    """Trajectories of 0 to 3 grains -- a union of one, empty ones first, in the middle and last, a grain on every offset: the
    edges left out are those of the first grain of every trajectory that has grains, on the source and on the destination side."""
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    og = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ng, nj = int(og[-1]), 5
    first = og[:-1][np.diff(og) > 0]
    rs = np.random.RandomState(len(sizes))
    gj = np.stack([np.repeat(np.arange(ng), 3), rs.randint(0, nj, 3 * ng)]).astype(np.int64)   # (every grain has edges)
    jg = np.ascontiguousarray(gj[::-1])
    dev = lambda a: torch.from_numpy(a).to(DEV)
    og_dev = dev(og)
    built = be.build_csr_batch([(dev(gj), ng, nj), (dev(jg), nj, ng)], masks=[(0, -1), (-1, 0)],
                               unions=[(og_dev, None), (None, og_dev)])
    _check_masked_union(be, built[0], gj, ng, nj, first, 0)
    _check_masked_union(be, built[1], jg, nj, ng, first, 1)


# ---- GPU: the boundary step of a union --------------------------------------------------------------------------------------

def _fixture_part(d, seed, spread=0.03):
    """A fixture's junctions moved by up to `spread` of the domain (some leave it), its grains, its grain->joint list."""
    f, off = float(d["domain_factor"]), torch.from_numpy(d["domain_offset"].copy())
    xj, xg = torch.from_numpy(d["scaled_x_joint"].copy()), torch.from_numpy(d["scaled_x_grain"].copy())
    rs = np.random.RandomState(seed)
    xj[:, :2] += torch.from_numpy(rs.uniform(-spread, spread, (xj.shape[0], 2)).astype(np.float32)) * f
    xg[:, :] += torch.from_numpy(rs.uniform(0.1, 0.2, tuple(xg.shape)).astype(np.float32))   # (nothing is zero before the reset)
    return dict(xj=xj, xg=xg, gj=torch.from_numpy(d["ei_" + etk(GJ)].copy()), off=off)


def _hand_made_part(n_grain, n_joint, n_boundary, seed):
    """Grain 0 holds the first `n_boundary` junctions (in a shuffled list); every junction also belongs to an inner grain."""
    rs = np.random.RandomState(seed)
    src = np.concatenate([np.zeros(n_boundary, np.int64), rs.randint(1, n_grain, n_joint)])
    dst = np.concatenate([np.arange(n_boundary), np.arange(n_joint)])
    order = rs.permutation(len(src))
    xj = torch.from_numpy(rs.uniform(-0.1, 1.1, (n_joint, 8)).astype(np.float32))
    xg = torch.from_numpy(rs.uniform(0.1, 0.9, (n_grain, 11)).astype(np.float32))
    return dict(xj=xj, xg=xg, gj=torch.from_numpy(np.stack([src[order], dst[order]])), off=torch.zeros(n_joint, 2))


def _run_boundary_union(parts, f, max_y=1.0):
    """`parts`: per trajectory a dict (xj, xg, gj, off) or None (empty).  The device's union call against
    _boundary_reference applied trajectory by trajectory; returns the number of junctions the step moved."""
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    real = [p for p in parts if p is not None]
    gj, jg, og, oj = _union_lists([None if p is None else (p["gj"].numpy(), p["gj"].numpy()[::-1], p["xg"].shape[0], p["xj"].shape[0])
                                   for p in parts])
    ref_j, ref_g = [p["xj"].clone() for p in real], [p["xg"].clone() for p in real]
    for p, rj, rg in zip(real, ref_j, ref_g):
        _boundary_reference(rj, rg, p["gj"], p["off"] if f > 1 else 0, f, max_y)
    XJ, XG = torch.cat([p["xj"] for p in real]), torch.cat([p["xg"] for p in real])
    off = torch.cat([p["off"] for p in real])
    xj, xg = XJ.to(DEV), XG.to(DEV)
    csr = be.build_csr(torch.from_numpy(jg).to(DEV), xj.size(0), xg.size(0))
    before = torch.empty(xj.size(0), 2, device=DEV)
    be.noflux_boundary(csr, xj, xg, f, off.to(DEV) if f > 1 else None, max_y, joints_before=before,
                       traj_offsets=(torch.from_numpy(og).to(DEV), torch.from_numpy(oj).to(DEV)))
    assert torch.equal(before.cpu(), XJ[:, :2]), "joints_before must receive the inputs"
    assert torch.equal(xj.cpu(), torch.cat(ref_j))
    assert torch.equal(xg.cpu(), torch.cat(ref_g))
    # every boundary grain is reset, no other grain row is touched
    bnd = check_noflux_union(og, oj)
    got, inner = xg.cpu(), np.setdiff1d(np.arange(xg.size(0)), bnd)
    assert torch.equal(got[inner], XG[inner])
    for g in bnd:
        assert got[g, [0, 1, 3, 4, 10]].tolist() == [0.5, 0.5, 0.0, 0.0, 0.0] and torch.equal(got[g, [2, 5, 6, 7, 8, 9]], XG[g, [2, 5, 6, 7, 8, 9]])
    return int((xj.cpu()[:, :2] != XJ[:, :2]).any(1).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["three_40um", "two_80um_folded", "empty_in_the_middle", "long_boundary_row"])
def test_boundary_step_of_a_union_is_bit_equal_to_the_reference_per_trajectory(case):
    """No node count here is a multiple of 256: every block straddles trajectories.  long_boundary_row: the middle
    trajectory's boundary grain has 1 100 junctions (> BND_CHUNK = 1024: two rounds of the chunk loop and its barriers) while
    its neighbours in the same blocks have 12 and 9 (one round)."""
    d40, d80 = fixture(F40), fixture(F80)
    if case == "three_40um":
        moved = _run_boundary_union([_fixture_part(d40, s) for s in (1, 2, 3)], 1.0)
    elif case == "two_80um_folded":
        assert float(d80["domain_factor"]) == 2.0
        moved = _run_boundary_union([_fixture_part(d80, s) for s in (4, 5)], 2.0)
    elif case == "empty_in_the_middle":
        moved = _run_boundary_union([_fixture_part(d40, 6), None, _fixture_part(d40, 7), None], 1.0)
    else:
        parts = [_hand_made_part(5, 40, 12, 1), _hand_made_part(4, 1150, 1100, 2), _hand_made_part(6, 30, 9, 3)]
        moved = _run_boundary_union(parts, 1.0, max_y=0.75)
    assert moved >= 30


@pytest.mark.gpu
@pytest.mark.parametrize("name", [F40, F80])
def test_grain_centres_of_a_noflux_union_equal_each_trajectorys_own_call(name):
    """ggnn_grain_centres(GGNN_BC_NOFLUX) is per grain on the full table and knows no grain 0: two perturbed trajectories as
    one union give each trajectory's own result, boundary grains included."""
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    d = fixture(name)
    f = float(d["domain_factor"])
    parts = [_fixture_part(d, s, 0.01) for s in (8, 9)]
    jg = [torch.from_numpy(np.ascontiguousarray(p["gj"].numpy()[::-1])) for p in parts]
    own = []
    for p, e in zip(parts, jg):
        xj, xg = p["xj"].to(DEV), p["xg"].to(DEV)
        be.grain_centres(be.build_csr(e.to(DEV), xj.size(0), xg.size(0)), xj, xg, f, p["off"].to(DEV) if f > 1 else None,
                         boundary="noflux")
        own.append(xg.cpu())
    assert not torch.equal(own[0][:, :2], parts[0]["xg"][:, :2])
    ng, nj = parts[0]["xg"].shape[0], parts[0]["xj"].shape[0]
    xj, xg = torch.cat([p["xj"] for p in parts]).to(DEV), torch.cat([p["xg"] for p in parts]).to(DEV)
    e = torch.cat([jg[0], jg[1] + torch.tensor([[nj], [ng]])], dim=1).to(DEV)
    off = torch.cat([p["off"] for p in parts]).to(DEV)
    be.grain_centres(be.build_csr(e, 2 * nj, 2 * ng), xj, xg, f, off if f > 1 else None, boundary="noflux")
    assert torch.equal(xg.cpu(), torch.cat(own))


# ---- GPU: rollouts --------------------------------------------------------------------------------------------------------------

def nf_rollout(d, graphs, use_graph, events=True, qoi=False, union=True, plan=None, thresholds=None):
    """GrainRollout(boundary="noflux") on the trajectories `graphs` of fixture `d`: a union with constructor offsets
    (`union`), or the one trajectory's own rollout.  -> (rollout, X, slices)."""
    from graingraphnn_amd import GrainRollout
    R, Cm = product_models(int(d["weight_seed"]), 1.0, DEV)
    x, ei, ea, slices = synthetic.disjoint_union(graphs)
    X = tt(x, DEV)
    f = float(d["domain_factor"])
    off = torch.from_numpy(np.concatenate([d["domain_offset"]] * len(graphs))).to(DEV) if f > 1 else None
    kw = {} if plan is None else dict(joint_launches=plan == "joint", concurrent=plan != "single")
    if union:
        kw["traj_offsets"] = offsets_of(slices)
    ro = GrainRollout(R, Cm, X, tt(ei, DEV), tt(ea, DEV), int(d["span"]), use_graph=use_graph, refresh_centres=True,
                      domain_factor=f, domain_offset=off, boundary="noflux", max_y=float(d["max_y"]), **kw)
    if events:
        mask = {k: np.concatenate([d["mask_" + k]] * len(graphs)) for k in ("grain", "joint")}
        thr = thresholds or (float(d["area_threshold"]), float(d["edge_threshold"]))
        ro.enable_events(mask, *thr)
    if qoi:
        ro.enable_qoi(capacity=40, **QOI_KW)
    return ro, X, slices


def nf_run_alone(d, graph, n_steps, use_graph, qoi):
    """test_ensemble_events.run_alone for a no-flux trajectory, with the QoI rows after every step:
    ((steps, ended_at, final state, message), [qoi rows per completed step])."""
    from graingraphnn_amd.topology import TopologyError
    ro, X, _ = nf_rollout(d, [graph], use_graph, qoi=qoi, union=False)
    steps, q = [], []
    final = lambda: snapshot(X["joint"], X["grain"], ro.mask, ro.edge_index, qoi_rows(ro.qoi()) if qoi else None)
    for _ in range(n_steps):
        try:
            _, ev, sw = ro.step_events()
        except TopologyError as err:
            return (steps, ro.steps_done, final(), str(err)), q
        steps.append((snapshot(X["joint"], X["grain"], ro.mask, ro.edge_index), ev.copy(), sw.copy()))
        if qoi:
            q.append(qoi_rows(ro.qoi()))
    return (steps, None, final(), None), q


# perturbations of the 40 um fixture's junctions to pick the union's middle trajectory from: (seed, sigma)
PERTURBATIONS = ((1000, 2e-3), (7, 5e-3), (11, 1e-2), (3, 2e-2))


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
@torch.no_grad()
def test_union_equals_the_trajectories_own_rollouts_and_the_reference(use_graph):
    """[40 um fixture, a perturbed copy, the fixture again] through 6 step_events() with the QoI on: after every step every
    trajectory's rows of x, masks, local lists, events and QoI are those of its own GrainRollout(boundary="noflux"), bit for
    bit, and trajectories 0 and 2 reproduce the reference's recorded trajectory."""
    d = fixture(F40)
    steps = int(d["steps"])
    assert steps == 6
    base, base_q = nf_run_alone(d, nf_graph(d), steps, use_graph, True)
    assert base[1] is None, "trajectory 0 must run all 6 steps"
    events_of = lambda a: [sorted(ev.tolist()) + [len(sw)] for _, ev, sw in a[0]]
    picked = None
    for seed, sigma in PERTURBATIONS:   # (the first whose event sequence is not the fixture's)
        g = nf_graph(d, seed, sigma)
        a, q = nf_run_alone(d, g, steps, use_graph, True)
        print(f"perturbation {(seed, sigma)}: events per step {events_of(a)}, ended at {a[1]}")
        if events_of(a) != events_of(base)[:len(a[0])] and sum(len(ev) for _, ev, _ in a[0]) > 0:
            picked = (g, a, q)
            break
    assert picked is not None, "no perturbed copy whose event sequence differs from the fixture's at some step"
    graphs = [nf_graph(d), picked[0], nf_graph(d)]
    alone, alone_q = [base, picked[1], base], [base_q, picked[2], base_q]
    assert sum(sum(len(ev) for _, ev, _ in a[0]) > 0 for a in alone) >= 2, "eliminations in at least two trajectories"
    ro, X, slices = nf_rollout(d, graphs, use_graph, qoi=True)
    assert ro._ens is not None and ro._ens["n_traj"] == 3
    compared = {"golden": 0, "qoi": 0}

    def after_step(step, events, switches):
        states, q = ro.trajectory_states(), ro.qoi()
        for t in range(3):
            (g0, g1), (j0, j1) = slices[t]["grain"], slices[t]["joint"]
            assert int(ro._live_grain[g0]) == 1 and int(ro._cand_grain[g0]) == 0 and g0 not in events
            if states[t]["ended_at"] is None:
                assert_same_state(qoi_rows(q, g0, g1, t), alone_q[t][step], f"QoI of trajectory {t} after step {step}")
                compared["qoi"] += 1
        assert torch.equal(ro._cand_grain.cpu()[np.setdiff1d(np.arange(ro._live_grain.numel()), [s["grain"][0] for s in slices])],
                           ro._live_grain.cpu()[np.setdiff1d(np.arange(ro._live_grain.numel()), [s["grain"][0] for s in slices])])
        for t in (0, 2):   # the reference's recorded trajectory
            (g0, g1), (j0, j1) = slices[t]["grain"], slices[t]["joint"]
            s, st = step + 1, states[t]
            mine = events[(events >= g0) & (events < g1)] - g0
            assert sorted(mine.tolist()) == sorted(d[f"s{s}_grain_event"].tolist()), (t, s)
            mine_sw = switches[(switches[:, 0] >= j0) & (switches[:, 0] < j1)]
            assert len(mine_sw) == len(d[f"s{s}_switching_list"]), (t, s)
            for et in EDGE_TYPES:
                assert np.array_equal(st["edge_index"][et], d[f"s{s}_ei_" + etk(et)]), (t, s, et)
            assert np.array_equal(st["mask"]["grain"], d[f"s{s}_mask_grain"]) and np.array_equal(st["mask"]["joint"], d[f"s{s}_mask_joint"])
            _check_state(None, {"joint": st["x_joint"], "grain": st["x_grain"]}, d, s, f"trajectory {t}")
            compared["golden"] += 1

    check_union_against_own_rollouts(ro, slices, alone, steps, True, after_step)
    assert compared["golden"] == 12 and compared["qoi"] >= 12
    assert ro.trajectory_states()[0]["ended_at"] is None
    with pytest.raises(_lib.GGNNError, match="step_events"):
        ro.run_events(1)


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["joint", "overlapped"])
@torch.no_grad()
def test_folded_union_on_the_static_plans(plan):
    """Two 80 um trajectories (folded by 2), the second perturbed: step(), and run(2) with RUN_UNROLL = 2, replayed from
    hipGraphs, equal the trajectories' own rollouts bit for bit; the first is the reference's quiet steps 1-2."""
    d = fixture(F80)
    graphs = [nf_graph(d), nf_graph(d, 5, 2e-3)]

    def advance(gs, union, how):
        ro, X, slices = nf_rollout(d, gs, True, events=False, union=union, plan=plan)
        ro.RUN_UNROLL = 2
        ro.step() if how == "step" else ro.run(2)
        return ro, X, slices
    for how, golden_step in (("step", 1), ("run", 2)):
        ro, X, slices = advance(graphs, True, how)
        assert ro._traj is not None and ro._pipelined() == (plan == "overlapped")
        for t, g in enumerate(graphs):
            _, X1, _ = advance([g], False, how)
            (g0, g1), (j0, j1) = slices[t]["grain"], slices[t]["joint"]
            assert torch.equal(X["joint"][j0:j1], X1["joint"]) and torch.equal(X["grain"][g0:g1], X1["grain"]), (how, t)
        (g0, g1), (j0, j1) = slices[0]["grain"], slices[0]["joint"]
        _check_state(None, {"joint": X["joint"][j0:j1], "grain": X["grain"][g0:g1]}, d, golden_step, f"{plan} {how}")
        assert not torch.equal(X["joint"][slices[1]["joint"][0]:], X["joint"][j0:j1])
        state = ro.state()
        assert torch.equal(state["joint_xy"], X["joint"][:, :2])
        assert all(torch.isfinite(v).all() for v in ro.edge_attr_dict().values())


@pytest.mark.gpu
@torch.no_grad()
def test_boundary_grains_never_make_a_union_step_eventful():
    """Two copies of the 40 um fixture with the area threshold between the boundary grains' predicted area and every interior
    grain's (test_noflux.test_boundary_grain_never_makes_a_step_eventful): the counts read back are all zero and
    step_events() takes the quiet path; counted against the live mask instead, every boundary grain would fire."""
    from graingraphnn_amd.backend import default_backend
    d = fixture(F40)
    area = torch.from_numpy(d["s1_pred_grain_area"])
    thr = float((area[0] + area[1:].min()) / 2)
    assert float(area[0]) < thr < float(area[1:].min())
    ro, X, slices = nf_rollout(d, [nf_graph(d), nf_graph(d)], False, thresholds=(thr, 0.99))
    _, ev, sw = ro.step_events()
    assert ro._ev_host.tolist() == [0] * 6, "the [2 + 2 n_traj] count words"
    assert len(ev) == 0 and len(sw) == 0 and ro._ens["rewired"] == 0 and ro._quiet_steps == 1
    E, p = ro._ens, ro.pred
    words = torch.zeros(6, dtype=torch.int32, device=DEV)
    for mask, want in ((ro._cand_grain, [0, 0, 0, 0, 0, 0]), (ro._live_grain, [2, 0, 1, 0, 1, 0])):
        default_backend().detect_events_traj(p["grain_area"], mask, thr, p["edge_event"], ro.edge_index[JJ], 10.0,
                                             E["grain_off"], E["joint_off"], words[2:], words[:2])
        assert words.cpu().tolist() == want


@pytest.mark.gpu
@torch.no_grad()
def test_rollout_trajectories_noflux_with_events_and_qoi():
    """dist.rollout_trajectories(boundary="noflux", events=..., qoi=...) in one process on four trajectories: every row is
    the trajectory's own rollout; ended_at and n_eliminated agree with the masks."""
    from graingraphnn_amd.dist import rollout_trajectories
    d = fixture(F40)
    steps = int(d["steps"])
    graphs = [nf_graph(d), nf_graph(d, 1000, 2e-3), nf_graph(d, 7, 5e-3), nf_graph(d)]
    R, Cm = product_models(int(d["weight_seed"]), 1.0, DEV)
    masks = [{"grain": d["mask_grain"], "joint": d["mask_joint"]}] * 4
    res = rollout_trajectories(R, Cm, graphs, int(d["span"]), steps, 0, 1, DEV, refresh_centres=True,
                               qoi=dict(QOI_KW, capacity=40), boundary="noflux", max_y=float(d["max_y"]),
                               events=dict(area_threshold=float(d["area_threshold"]), edge_threshold=float(d["edge_threshold"]),
                                           mask=masks))
    assert set(res) == {"joint_xy", "grain_area_v", "volume", "size", "grain_live", "joint_live", "ended_at", "n_eliminated"}
    n_g, n_j = d["x_grain"].shape[0], d["x_joint"].shape[0]
    assert res["grain_live"].shape == (4, n_g) and res["joint_live"].shape == (4, n_j) and res["ended_at"].shape == (4,)
    for t, g in enumerate(graphs):
        (_, ended_at, final, _), _ = nf_run_alone(d, g, steps, True, True)
        assert int(res["ended_at"][t]) == (-1 if ended_at is None else ended_at), t
        live = (final["mask_grain"][:, 0] > 0).astype(np.float32)
        want = {"joint_xy": final["x_joint"][:, :2], "grain_area_v": final["x_grain"][:, 3:5], "volume": final["volume"],
                "size": final["size"], "grain_live": live, "joint_live": (final["mask_joint"][:, 0] > 0).astype(np.float32)}
        for key, v in want.items():
            assert np.array_equal(res[key][t].cpu().numpy(), v, equal_nan=True), (t, key)
        assert float(res["n_eliminated"][t]) == n_g - live.sum() == n_g - float(res["grain_live"][t].sum()), t
        assert float(res["grain_live"][t][0]) == 1.0, "the boundary grain stays"
    gone = n_g - int((d[f"s{steps}_mask_grain"] > 0).sum())   # (the reference's trajectory: 40 grains in 41 events, one forced twice)
    assert int(res["ended_at"][0]) == -1 and float(res["n_eliminated"][0]) == gone == 40 and float(res["n_eliminated"].min()) > 0
    # static topology: the union's run() against the trajectories' own
    res = rollout_trajectories(R, Cm, graphs[:2], int(d["span"]), 2, 0, 1, DEV, refresh_centres=True, boundary="noflux",
                               max_y=float(d["max_y"]))
    assert set(res) == {"joint_xy", "grain_area_v"}
    for t, g in enumerate(graphs[:2]):
        ro, X, _ = nf_rollout(d, [g], True, events=False, union=False)
        ro.run(2)
        assert torch.equal(res["joint_xy"][t], X["joint"][:, :2]) and torch.equal(res["grain_area_v"][t], X["grain"][:, 3:5]), t


@pytest.mark.gpu
@torch.no_grad()
def test_refusals_of_a_noflux_union():
    d = fixture(F40)
    ro, X, slices = nf_rollout(d, [nf_graph(d), nf_graph(d)], False, events=False)
    off = offsets_of(slices)
    mask = {k: np.concatenate([d["mask_" + k]] * 2) for k in ("grain", "joint")}
    other = {"grain": [0, 100, 202], "joint": off["joint"]}
    with pytest.raises(_lib.GGNNError, match="differ"):
        ro.enable_events(mask, 1e-4, 0.6, traj_offsets=other)
    with pytest.raises(_lib.GGNNError, match="differ"):
        ro.enable_qoi(**QOI_KW, traj_offsets=[0, 202])
    ro.enable_events(mask, 1e-4, 0.6, traj_offsets=off)   # (equal ones are accepted)
    ro.enable_qoi(**QOI_KW, traj_offsets=off["grain"])
    assert ro._ens["n_traj"] == 2 and ro._qoi["offsets_host"].tolist() == off["grain"]
    with pytest.raises(_lib.GGNNError, match="step_events"):
        ro.run_events(1)
    # a single no-flux rollout still says where a union's offsets go
    one, _, _ = nf_rollout(d, [nf_graph(d)], False, events=False, union=False)
    with pytest.raises(_lib.GGNNError, match="noflux.*construct"):
        one.enable_events({"grain": d["mask_grain"], "joint": d["mask_joint"]}, 1e-4, 0.6,
                          traj_offsets={"grain": [0, 101], "joint": [0, 198]})


# The C-ABI calls of one step_events() of a single no-flux rollout (eager launches, grain centres refreshed) behind the two
# forwards, as the rollout made them before no-flux unions existed: a quiet step, and an eventful one.
QUIET_STEP = ["ggnn_heads_regressor", "ggnn_heads_classifier", "ggnn_step_update", "ggnn_detect_events", "ggnn_noflux_boundary",
              "ggnn_grain_centres", "ggnn_step_refresh"]
EVENTFUL_STEP = QUIET_STEP[:4] + ["ggnn_build_csr_batch"] + QUIET_STEP[4:]


@pytest.mark.gpu
@torch.no_grad()
def test_off_means_off():
    """A single no-flux rollout without offsets never reaches a *_traj entry point and makes, step for step, the calls it
    made before; with one-trajectory offsets the only differences are those entry points, and x comes out bit-equal."""
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    d = fixture(F40)

    def counted(union):
        ro, X, _ = nf_rollout(d, [nf_graph(d)], False, union=union)
        lib, per_step = be.lib, []
        try:
            for _ in range(int(d["steps"])):
                be.lib = counting = _CountingLib(lib)
                ro.step_events()
                per_step.append(counting.calls)
        finally:
            be.lib = lib
        return per_step, ro
    off, ro_off = counted(False)
    print("entry points per step without traj_offsets:", off)
    assert ro_off._ens is None and ro_off._traj is None and ro_off._cand_grain is ro_off._live_grain
    eventful = [len(e) > 0 or len(s) > 0 for e, s in zip(ro_off.grain_events, ro_off.switched)]
    assert eventful == [False, True, True, True, True, True]
    n_fwd = off[0].index("ggnn_heads_regressor")
    assert n_fwd >= 2 and off[0][0] == "ggnn_edge_prepare" and all(c[:n_fwd] == off[0][:n_fwd] for c in off)
    assert [c[n_fwd:] for c in off] == [QUIET_STEP] + [EVENTFUL_STEP] * 5
    on, ro_on = counted(True)
    swap = {"ggnn_detect_events": "ggnn_detect_events_traj", "ggnn_noflux_boundary": "ggnn_noflux_boundary_traj",
            "ggnn_build_csr_batch": "ggnn_build_csr_batch_traj"}
    assert on == [[swap.get(c, c) for c in calls] for calls in off]
    for nt in ("joint", "grain"):
        assert torch.equal(ro_on.x[nt], ro_off.x[nt]), nt
