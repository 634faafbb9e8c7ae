"""The layers' grain polygons recorded on the device during rollouts (ggnn_grain_polygons, GrainRollout.enable_polygons /
polygons) against the numpy restatement of tests/polycheck.py and the reference's own `regions` / `region_coors` /
`region_center` (tests/golden/make_golden_polygons.py).

The contract (polycheck): against the REFERENCE the cyclic sequence of every grain whose smallest angular gap is at least
1e-3 rad, the start vertex where the seam distance exceeds 1e-4 rad, the centres within the bound of the centre goldens
(helpers.assert_close), the coordinates within one float32 rounding of a shifted coordinate (2^-23: the reference moves
periodic vertices in float64); against the float32 RESTATEMENT joint_sorted, xy_sorted and centre bit for bit and the area
within polycheck.area_bound."""
import os

import numpy as np
import pytest
import torch

import polycheck
from helpers import EDGE_TYPES, GOLDEN, assert_close, etk, load_graph, product_models, tt
from graingraphnn_amd import _lib

GJ, JG, JJ = EDGE_TYPES
DEV = "cuda"
COOR_TOL = 2.0 ** -23
TAGS = ("init", "step1", "step3", "mass3", "noflux")


def npz(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def golden_case(tag):
    """(x_joint, joint->grain list, boundary, n_grain, regions per grain or None, coors, centre) of a recorded state."""
    G = npz("polygons_cfg1")
    if tag == "noflux":
        d = npz("noflux_40_seed1")
        xj, ei, bc = d["scaled_x_joint"], d["ei_" + etk(JG)], "noflux"
    elif tag == "mass3":
        d = npz("golden_cfg1_events")
        xj, ei, bc = d["mass3__out_x_joint"], d["mass3__out_ei_" + etk(JG)], "periodic"
    else:
        g40 = npz("graph_40")
        xj = g40["x_joint"] if tag == "init" else npz("golden_cfg1_centres")[f"{tag}_x_joint"]
        ei, bc = g40["ei_" + etk(JG)], "periodic"
    rp = G[tag + "__rowptr"]
    regions = [G[tag + "__regions"][rp[g]:rp[g + 1]] if rp[g + 1] > rp[g] else None for g in range(len(rp) - 1)]
    coors = [G[tag + "__coors"][rp[g]:rp[g + 1]] for g in range(len(rp) - 1)]
    return xj, ei, bc, len(rp) - 1, regions, coors, G[tag + "__center"]


def assert_contract(joint_sorted, xy_sorted, centre, rowptr, cls, regions, coors, ref_centre, what, max_excluded=0,
                    max_excluded_share=None):
    """The contract against the reference's record of the same topology (module docstring)."""
    c = polycheck.compare_with_reference(joint_sorted, rowptr, regions, cls)
    print(what, {k: v for k, v in c.items()})
    assert c["compared"] > 0 and not c["cyclic_bad"] and not c["start_bad"], (what, c)
    if max_excluded_share is None:
        assert len(c["excluded"]) <= max_excluded, (what, c["excluded"])
    else:
        assert len(c["excluded"]) <= max_excluded_share * (c["compared"] + len(c["excluded"])), (what, c["excluded"])
    has = np.isfinite(ref_centre[:, 0])
    assert_close(np.asarray(centre)[has], ref_centre[has].astype(np.float32), what + " centres")
    if coors is None:
        return
    worst = 0.0
    for g, ref in enumerate(regions):
        if ref is None or g in c["excluded"]:
            continue
        p0, p1 = int(rowptr[g]), int(rowptr[g + 1])
        rot = polycheck.rotation_of([int(v) for v in ref], [int(v) for v in joint_sorted[p0:p1]])
        got = np.roll(np.asarray(xy_sorted[p0:p1], np.float64), -rot, axis=0)
        worst = max(worst, float(np.abs(got - coors[g]).max()))
    print(what, "worst coordinate difference", worst)
    assert worst <= COOR_TOL, (what, worst)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference(tag):
    """Both restatements on the recorded inputs: the cyclic order for ALL grains (no grain of these states is below the gap
    limit; the no-flux fixture may exclude 2), the start vertex under the seam rule, centres and coordinates."""
    xj, ei, bc, n, regions, coors, centre = golden_case(tag)
    rowptr, col = polycheck.table_of(ei, n)
    assert all((r is None) == (rowptr[g + 1] - rowptr[g] < 2) for g, r in enumerate(regions))
    cls = polycheck.classify(rowptr, col, xj, boundary=bc)
    for dtype in (np.float64, np.float32):
        r = polycheck.restate(rowptr, col, xj, boundary=bc, dtype=dtype)
        assert_contract(r["joint_sorted"], r["xy_sorted"], r["centre"], rowptr, cls, regions, coors, centre,
                        f"{tag} {dtype.__name__}", max_excluded=2 if tag == "noflux" else 0)
        for g in range(n):   # a permutation of the row, row by row
            assert sorted(r["joint_sorted"][rowptr[g]:rowptr[g + 1]]) == sorted(col[rowptr[g]:rowptr[g + 1]])
    if tag == "noflux":   # the boundary grain runs clockwise: negative area, the rest positive
        assert r["sides"][0] == 38 and r["area"][0] < 0 and (r["area"][1:] > 0).all()
        assert np.all(np.abs(r["area"]) <= r["area_terms"])


def test_the_contract_rejects_a_wrong_order_and_a_wrong_start():
    xj, ei, bc, n, regions, coors, centre = golden_case("step1")
    rowptr, col = polycheck.table_of(ei, n)
    cls = polycheck.classify(rowptr, col, xj, boundary=bc)
    good = polycheck.restate(rowptr, col, xj, boundary=bc)["joint_sorted"]
    clockwise, rotated, swapped = good.copy(), good.copy(), good.copy()
    p0, p1 = int(rowptr[5]), int(rowptr[6])
    clockwise[p0:p1] = good[p0:p1][::-1]
    rotated[p0:p1] = np.roll(good[p0:p1], 1)
    swapped[p0], swapped[p0 + 1] = good[p0 + 1], good[p0]
    assert cls["seam"][5] > polycheck.SEAM_MIN
    assert polycheck.compare_with_reference(clockwise, rowptr, regions, cls)["cyclic_bad"] == [5]
    assert polycheck.compare_with_reference(swapped, rowptr, regions, cls)["cyclic_bad"] == [5]
    c = polycheck.compare_with_reference(rotated, rowptr, regions, cls)
    assert c["cyclic_bad"] == [] and c["start_bad"] == [5]


def test_entry_point_validates_on_the_host():
    import ctypes
    lib = _lib.load()
    assert ctypes.sizeof(_lib.PolygonArgs) == 14 * 8 + 6 * 8 + 2 * 4
    assert lib.ggnn_grain_polygons(None, None) == -1
    assert lib.ggnn_grain_polygons(ctypes.byref(_lib.PolygonArgs()), None) == -1
    buf = (ctypes.c_float * 64)()                 # (host memory: refused before anything would be launched)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def args(**kw):
        A = _lib.PolygonArgs(p, p, p, None, None, p, p, p, p, p, None, None, None, None, 4, 2, 3, 9, 1, 0, 1.0, _lib.BC_PERIODIC)
        for k, v in kw.items():
            setattr(A, k, v)
        return ctypes.byref(A)
    for bad in (dict(boundary=7), dict(domain_factor=0.5), dict(ldx_joint=1), dict(n_grain=0), dict(n_traj=2), dict(capacity=-1),
                dict(E_cap=-1), dict(rowptr=None), dict(area=None), dict(layer_out=p), dict(traj_grain_off=p, n_traj=0)):
        assert lib.ggnn_grain_polygons(args(**bad), None) == -1, bad


def test_rollout_refuses_polygons_before_they_are_enabled():
    from graingraphnn_amd import GrainRollout
    ro = object.__new__(GrainRollout)
    ro._poly = None
    with pytest.raises(_lib.GGNNError):
        ro.polygons()
    ro._enqueue_polygons()   # off: no launch, nothing touched (the object has no backend at all)


# ---- GPU: the kernel alone ------------------------------------------------------------------------------------------------

ROWS = (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 70)       # grains 4..7 share a wave: two of its rows take the wave's path
STRADDLERS = ((0.995, 0.4, 6), (0.3, 0.004, 7), (0.998, 0.997, 5), (0.003, 0.5, 9), (0.5, 0.999, 12), (0.002, 0.001, 8))
EQUAL_ANGLE = len(ROWS) + len(STRADDLERS)             # the grain with two vertices at angle 0 and two at pi
TRAJ_OFF = (0, 4, 4, 7, EQUAL_ANGLE, EQUAL_ANGLE + 31)  # an empty trajectory; first grains with 0, 15, 63 and 6 junctions


def synthetic_rows(boundary, factor, seed=11):
    """Grains with junctions of their own on perturbed circles, the vertices of a row in random order, junction ids and
    the list's columns shuffled.  periodic: coordinates wrapped into [0, 1); no-flux: as they are (a polygon that reaches
    below 0 takes the +1 shift without a chain).  factor > 1: the state as scale_feature_patchs folds it.
    -> (x_joint [n_joint, 8], list [2, E], n_grain, domain_offset or None)"""
    rs = np.random.RandomState(seed)
    polys = []
    for n in ROWS:
        c = rs.uniform(0.3, 0.7, 2) if boundary == "noflux" else rs.uniform(0.0, 1.0, 2)
        polys.append((n, c, rs.uniform(0.05, 0.2)))
    polys += [(n, np.array([cx, cy]), rs.uniform(0.03, 0.1)) for cx, cy, n in STRADDLERS]
    rows = []
    for n, c, rad in polys:
        ang = 2 * np.pi * (np.arange(n) + 0.35 * rs.uniform(-1, 1, n)) / max(n, 1) + rs.uniform(0, 2 * np.pi)
        r = rad * (1 + 0.2 * rs.uniform(-1, 1, n))
        rows.append((c + np.stack([r * np.cos(ang), r * np.sin(ang)], 1))[rs.permutation(n)])
    # centre exactly (0.5, 0.5) in float32 (dyadic coordinates, exact partial sums): angle 0 and angle pi twice each
    rows.append(np.array([[0.75, 0.5], [0.25, 0.5], [0.5, 0.75], [0.625, 0.5], [0.5, 0.25], [0.375, 0.5]]))
    for _ in range(30):   # the common case, and a third block
        n = rs.randint(3, 13)
        c, rad = rs.uniform(0.3, 0.7, 2), rs.uniform(0.03, 0.15)
        ang = 2 * np.pi * (np.arange(n) + 0.35 * rs.uniform(-1, 1, n)) / n + rs.uniform(0, 2 * np.pi)
        rows.append((c + rad * np.stack([np.cos(ang), np.sin(ang)], 1))[rs.permutation(n)])
    xy = np.concatenate(rows)
    if boundary == "periodic":
        xy = xy - np.floor(xy)
    grain = np.concatenate([np.full(len(r), g, np.int64) for g, r in enumerate(rows)])
    ids = rs.permutation(len(xy))
    xj = rs.uniform(-1, 1, (len(xy), 8)).astype(np.float32)
    xj[ids, :2] = xy.astype(np.float32)
    off = None
    if factor > 1:
        scaled = xj[:, :2] * np.float32(factor)
        off = np.floor(scaled).astype(np.float32)
        xj[:, :2] = scaled - off
    cols = rs.permutation(len(xy))
    return xj, np.stack([ids[cols], grain[cols]]), len(rows), off


def arena_numpy(arena, layer=0):
    out = {k: v[layer].cpu().numpy() for k, v in arena.items()}
    E = int(out["rowptr"][-1])
    out["joint_sorted"], out["xy_sorted"] = out["joint_sorted"][:E], out["xy_sorted"][:E]
    return out


def assert_equals_restatement(got, r, what):
    """joint_sorted, xy_sorted and centre bit for bit, the area within its bound (exactly 0 for rows of 0 or 1 junction)."""
    assert np.array_equal(got["joint_sorted"], r["joint_sorted"]), what
    assert np.array_equal(got["xy_sorted"].view(np.int32), r["xy_sorted"].view(np.int32)), what
    assert np.array_equal(got["centre"].view(np.int32), r["centre"].view(np.int32)), what
    assert np.isfinite(got["area"]).all() and not got["area"][r["sides"] < 2].any(), what
    err, bound = np.abs(got["area"].astype(np.float64) - r["area"]), polycheck.area_bound(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        print(what, "worst area error / bound:", float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    assert (err <= bound).all(), (what, np.flatnonzero(err > bound))


@pytest.mark.gpu
@pytest.mark.parametrize("boundary,factor,union", [("periodic", 1.0, False), ("periodic", 3.0, False), ("noflux", 1.0, False),
                                                   ("noflux", 1.0, True)])
def test_kernel_against_the_restatement_on_synthetic_rows(boundary, factor, union):
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    xj, ei, n_grain, off = synthetic_rows(boundary, factor)
    csr = be.build_csr(torch.from_numpy(ei).to(DEV), xj.shape[0], n_grain)
    traj = np.asarray(TRAJ_OFF, np.int64) if union else None
    assert traj is None or traj[-1] == n_grain
    arena = be.grain_polygons(csr, torch.from_numpy(xj).to(DEV), None, factor, None if off is None else torch.from_numpy(off).to(DEV),
                              boundary=boundary, traj_grain_off=None if traj is None else torch.from_numpy(traj).to(DEV))
    got = arena_numpy(arena)
    rowptr, col = csr.rowptr.cpu().numpy(), csr.col.cpu().numpy()
    assert np.array_equal(got["rowptr"], rowptr) and tuple(np.diff(rowptr)[:len(ROWS)]) == ROWS
    kw = dict(boundary=boundary, domain_factor=factor, domain_offset=off, traj_grain_off=traj)
    r = polycheck.restate(rowptr, col, xj, **kw)
    assert_equals_restatement(got, r, f"{boundary} x{factor:g}")
    # the float64 rule agrees wherever it can be told apart from rounding
    cls = polycheck.classify(rowptr, col, xj, **kw)
    r64 = cls["restated"]
    told = 0
    for g in range(n_grain):
        p0, p1 = rowptr[g], rowptr[g + 1]
        if p1 - p0 >= 2 and cls["gap"][g] >= polycheck.GAP_MIN:
            rot = polycheck.rotation_of(list(r64["joint_sorted"][p0:p1]), list(got["joint_sorted"][p0:p1]))
            assert rot is not None and (rot == 0 or cls["seam"][g] <= polycheck.SEAM_MIN), g
            told += 1
    assert told >= n_grain - 6
    # the length key: same angle, the shorter first -- at angle 0 (0.625 before 0.75) and at pi (0.375 before 0.25)
    p0 = rowptr[EQUAL_ANGLE]
    want = [[0.625, 0.5], [0.75, 0.5], [0.5, 0.75], [0.375, 0.5], [0.25, 0.5], [0.5, 0.25]]
    if factor == 1.0:
        order = want if not (union and EQUAL_ANGLE in TRAJ_OFF) else want[::-1]
        assert got["xy_sorted"][p0:p0 + 6].tolist() == order and tuple(got["centre"][EQUAL_ANGLE]) == (0.5, 0.5)
    # the shift and the chain were exercised, and the reversed grains run clockwise
    assert (got["xy_sorted"] > 1.0).any() and (boundary == "noflux" or (got["xy_sorted"] < 0.0).sum() == 0)
    reversed_ = polycheck.boundary_grains(n_grain, boundary, traj)
    assert reversed_ == (set() if boundary == "periodic" else ({0, 4, 7, EQUAL_ANGLE} if union else {0}))
    for g in range(n_grain):
        if rowptr[g + 1] - rowptr[g] >= 3:
            assert (got["area"][g] < 0) == (g in reversed_), g


@pytest.mark.gpu
def test_kernel_layer_counter_and_capacity():
    """Rows follow the device-side counter; a layer beyond the capacity writes nothing (the guard row behind the arena
    stays), raises the overflow bit and still counts."""
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    xj, ei, n_grain, _ = synthetic_rows("periodic", 1.0)
    csr = be.build_csr(torch.from_numpy(ei).to(DEV), xj.shape[0], n_grain)
    X = torch.from_numpy(xj).to(DEV)
    big = be.polygon_arena(n_grain, csr.col.numel(), 3, DEV)
    for v in big.values():
        v.fill_(-7)
    arena = {k: v[:3] for k, v in big.items()}
    layer = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    words = torch.zeros(2, dtype=torch.int32, device=DEV)
    be.grain_polygons(csr, X, arena, layer_in=None, layer_out=layer, sync_word=words[:1], flags=words[1:])
    assert int(layer) == 0
    first = arena_numpy(arena, 0)
    for k in (1, 2):
        X[:, :2] += 0.001
        be.grain_polygons(csr, X, arena, layer_in=layer, layer_out=layer, sync_word=words[:1], flags=words[1:])
        assert int(layer) == k and words.tolist() == [0, 0]
    kept = {k: v.clone() for k, v in big.items()}
    be.grain_polygons(csr, X, arena, layer_in=layer, layer_out=layer, sync_word=words[:1], flags=words[1:])
    assert int(layer) == 3 and words.tolist() == [0, _lib.GGNN_FLAG_POLYGON_OVERFLOW]
    for k, v in big.items():
        assert torch.equal(v, kept[k]) and bool((v[3] == -7).all()), k
    again = arena_numpy(arena, 0)
    assert all(np.array_equal(first[k], again[k]) for k in first)
    assert not np.array_equal(arena_numpy(arena, 2)["xy_sorted"], first["xy_sorted"])
    with pytest.raises(_lib.GGNNError):
        be.grain_polygons(csr, X, arena, layer_in=layer, layer_out=layer)


# ---- GPU: rollouts -------------------------------------------------------------------------------------------------------

def record(ro, layer=None, traj=None):
    p = ro.polygons(layer, traj)
    out = {k: p[k].cpu().numpy().copy() for k in ("rowptr", "joint_sorted", "xy_sorted", "centre", "area", "sides")}
    out["layer"] = p["layer"]
    return out


def direct(ro):
    """The kernel called on the rollout's state as it is."""
    a = ro.be.grain_polygons(ro.graph.csr_full[JG], ro.x["joint"], None, ro.domain_factor, ro.domain_offset,
                             boundary=ro.boundary, traj_grain_off=ro._traj_grain_dev())
    out = arena_numpy(a)
    out["sides"] = np.diff(out["rowptr"])
    return out


def restated(ro, dtype=np.float32):
    csr = ro.graph.csr_full[JG]
    rowptr, col = csr.rowptr.cpu().numpy(), csr.col.cpu().numpy()
    kw = dict(boundary=ro.boundary, domain_factor=ro.domain_factor,
              domain_offset=None if ro.domain_offset is None else ro.domain_offset.cpu().numpy(),
              traj_grain_off=None if ro._traj is None else ro._traj["grain"])
    return rowptr, col, kw, polycheck.restate(rowptr, col, ro.x["joint"].cpu().numpy(), dtype=dtype, **kw)


def assert_same_record(a, b, what):
    for k in ("rowptr", "joint_sorted", "xy_sorted", "centre", "area", "sides"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def cfg1_rollout(polygons=6, **kw):
    from graingraphnn_amd import GrainRollout
    x, ei, ea = load_graph("40")
    R, Cm = product_models(10020, 1.0, DEV)
    X = tt(x, DEV)
    ro = GrainRollout(R, Cm, X, tt(ei, DEV), tt(ea, DEV), 6, refresh_centres=True, **kw)
    if polygons is not None:
        ro.enable_polygons(capacity=polygons)
    return ro, X


@pytest.mark.gpu
@torch.no_grad()
def test_golden_states_through_the_rollout():
    """Layer 0 and the layers of static steps 1 and 3 against the reference's record of those states."""
    ro, X = cfg1_rollout(polygons=3)
    for layer in range(4):
        if layer:
            ro.step()
        if layer == 2:
            continue
        tag = "init" if layer == 0 else f"step{layer}"
        _, _, _, n, regions, coors, centre = golden_case(tag)
        got = record(ro)
        assert got["layer"] == layer
        rowptr, col, kw, r = restated(ro)
        assert_equals_restatement(got, r, tag)
        cls = polycheck.classify(rowptr, col, X["joint"].cpu().numpy(), **kw)
        # (the rollout's junctions are the reference's to the parity bar, not bit for bit: the coordinates are compared
        #  through the restatement above, the order and the centres with the reference's record)
        assert_contract(got["joint_sorted"], got["xy_sorted"], got["centre"], rowptr, cls, regions, coors if layer == 0 else None,
                        centre, tag, max_excluded_share=0.01)
    assert ro.polygons()["layers"] == 3 and ro.polygons(layer=0)["layer"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["joint", "overlapped"])
@torch.no_grad()
def test_graph_replay_eager_steps_and_the_direct_call_agree(plan):
    """run(6) as two replays of a 3-step hipGraph (the layer counter lives on the device), six eager step()s and the kernel
    called on the state after every step: the same records bit for bit, each equal to the restatement; and the final state
    with the recorder on is the state with it off (the launch only reads)."""
    kw = dict(joint_launches=plan == "joint", concurrent=True)
    eager, Xe = cfg1_rollout(use_graph=False, **kw)
    by_hand = [direct(eager)]
    for k in range(1, 7):
        eager.step()
        by_hand.append(direct(eager))
        assert_equals_restatement(by_hand[-1], restated(eager)[3], f"{plan} step {k}")
    graphed, Xg = cfg1_rollout(use_graph=True, **kw)
    graphed.RUN_UNROLL = 3
    graphed.run(6)
    assert graphed.polygons()["layers"] == eager.polygons()["layers"] == 6
    for k in range(7):
        assert_same_record(record(eager, k), by_hand[k], (plan, "eager", k))
        assert_same_record(record(graphed, k), by_hand[k], (plan, "graph", k))
    assert not np.array_equal(by_hand[0]["xy_sorted"], by_hand[6]["xy_sorted"])
    off, Xo = cfg1_rollout(polygons=None, use_graph=True, **kw)
    off.RUN_UNROLL = 3
    off.run(6)
    for nt in Xe:
        assert torch.equal(Xe[nt], Xo[nt]) and torch.equal(Xg[nt], Xo[nt]), nt
    for et in EDGE_TYPES:
        assert torch.equal(eager.edge_attr_dict()[et], off.edge_attr_dict()[et]), et
    assert torch.equal(eager.state()["joint_xy"], off.state()["joint_xy"])


@pytest.mark.gpu
@torch.no_grad()
def test_events_step_by_step_and_speculative():
    """The seeded 40 um trajectory whose steps 3 and 4 eliminate 22 and 75 grains: every layer of step_events() equals the
    restatement on that step's topology and state -- layer 3 also the reference's record of that update -- and run_events()
    (speculative blocks from hipGraphs, the steps behind an eventful one voided and their rows written again) records the
    same layers bit for bit."""
    mask = {"grain": np.ones((118, 1)), "joint": np.ones((236, 1))}
    kw = dict(use_graph=True, joint_launches=False, concurrent=True)
    ra, Xa = cfg1_rollout(**kw)
    rb, Xb = cfg1_rollout(**kw)
    ra.enable_events(mask, 1e-4, 0.6)
    rb.enable_events(mask, 1e-4, 0.6)
    assert ra.polygons()["layers"] == 0   # (enable_events keeps the record)
    events, sides = [], []
    for k in range(1, 6):
        events.append(len(ra.step_events()[1]))
        got = record(ra)
        assert got["layer"] == k
        rowptr, col, kw_, r = restated(ra)
        assert_equals_restatement(got, r, f"step_events {k}")
        assert_same_record(got, direct(ra), ("direct", k))
        sides.append(got["sides"])
        if k == 3:
            _, _, _, n, regions, _, centre = golden_case("mass3")
            cls = polycheck.classify(rowptr, col, Xa["joint"].cpu().numpy(), **kw_)
            assert_contract(got["joint_sorted"], got["xy_sorted"], got["centre"], rowptr, cls, regions, None, centre, "mass3",
                            max_excluded_share=0.01)
    assert events[:4] == [0, 0, 22, 75]
    # an eliminated grain keeps an empty row: 22 after step 3, all but the 26 live grains after step 4
    assert (sides[2] == 0).sum() == 22 and (sides[3] == 0).sum() == 118 - 26 and sides[3].sum() < sides[1].sum()
    assert np.array_equal(sides[4] == 0, ra.mask["grain"][:, 0] == 0)
    for n in (3, 2):
        rb.run_events(n)
    for nt in Xa:
        assert torch.equal(Xa[nt], Xb[nt]), nt
    assert rb.polygons()["layers"] == 5
    for k in range(6):
        assert_same_record(record(ra, k), record(rb, k), ("run_events", k))


@pytest.mark.gpu
@torch.no_grad()
def test_union_records_equal_each_trajectorys_own():
    """A periodic union of three trajectories with events: polygons(traj=t) of every layer is that trajectory's own
    rollout's record bit for bit, junction ids local; a trajectory whose update is refused stops counting where its own
    rollout raised."""
    from graingraphnn_amd.topology import TopologyError
    from test_ensemble_events import cfg1, rollout_of, union_rollout
    graphs = [cfg1(), cfg1("perturbed", 1000, 1e-3), cfg1("perturbed", 7, 5e-3)]
    steps = 4
    ro, X, slices = union_rollout(graphs, True, False)
    ro.enable_polygons(capacity=steps)
    for _ in range(steps):
        ro.step_events()
    whole = ro.polygons()
    assert len(whole["layers"]) == 3 and whole["rowptr"].numel() == X["grain"].size(0) + 1
    for t, g in enumerate(graphs):
        alone, _ = rollout_of(g, True, False)
        alone.enable_polygons(capacity=steps)
        try:
            for _ in range(steps):
                alone.step_events()
        except TopologyError:
            pass
        layers = alone.polygons()["layers"]
        assert ro.polygons(traj=t)["layers"] == layers == int(whole["layers"][t]) and (layers == steps or t > 0)
        for k in range(layers + 1):
            a, u = record(alone, k), record(ro, k, traj=t)
            assert_same_record(a, u, (t, k))
            assert u["rowptr"][0] == 0 and (u["joint_sorted"].size == 0 or 0 <= u["joint_sorted"].min()
                                           and u["joint_sorted"].max() < slices[t]["joint"][1] - slices[t]["joint"][0])
        with pytest.raises(_lib.GGNNError):
            ro.polygons(layer=layers + 1, traj=t)
    with pytest.raises(_lib.GGNNError):
        ro.polygons(traj=3)


@pytest.mark.gpu
@torch.no_grad()
def test_noflux_union_reverses_every_trajectorys_boundary_grain():
    """Two 40 um no-flux trajectories (the fixture and a perturbed copy), two static steps: each trajectory's record is its
    own rollout's, equals the restatement with the union's offsets, and its boundary grain (38 sides: the wave's path) runs
    clockwise while every other grain runs counter-clockwise."""
    from test_noflux import fixture
    from test_noflux_ensemble import F40, nf_graph, nf_rollout
    d = fixture(F40)
    graphs = [nf_graph(d), nf_graph(d, 1000, 2e-3)]
    ro, X, slices = nf_rollout(d, graphs, False, events=False)
    ro.enable_polygons(capacity=2)
    for _ in range(2):
        ro.step()
        assert_equals_restatement(record(ro), restated(ro)[3], "noflux union")
    for t, g in enumerate(graphs):
        alone, _, _ = nf_rollout(d, [g], False, events=False, union=False)
        alone.enable_polygons(capacity=2)
        for _ in range(2):
            alone.step()
        for k in range(3):
            u = record(ro, k, traj=t)
            assert_same_record(record(alone, k), u, (t, k))
            assert u["sides"][0] == 38 and u["area"][0] < 0 and (u["area"][1:][u["sides"][1:] >= 3] > 0).all(), (t, k)
    # layer 0 of trajectory 0 is the reference's own record of the structure
    xj, ei, bc, n, regions, coors, centre = golden_case("noflux")
    u = record(ro, 0, traj=0)
    rowptr, col = polycheck.table_of(ei, n)
    assert np.array_equal(u["rowptr"], rowptr)
    assert_contract(u["joint_sorted"], u["xy_sorted"], u["centre"], rowptr, polycheck.classify(rowptr, col, xj, boundary=bc),
                    regions, coors, centre, "noflux layer 0", max_excluded=2)


@pytest.mark.gpu
@torch.no_grad()
def test_rollout_trajectories_hands_the_option_through():
    """dist.rollout_trajectories(polygons=True): the rank's own records, per trajectory those of its own rollout; the
    gathered keys are what they are without the option."""
    from graingraphnn_amd import dist
    from test_ensemble_events import cfg1
    graphs = [cfg1(), cfg1("perturbed", 1000, 1e-3)]
    R, Cm = product_models(10020, 1.0, DEV)
    plain = dist.rollout_trajectories(R, Cm, graphs, 6, 2, refresh_centres=True)
    out = dist.rollout_trajectories(R, Cm, graphs, 6, 2, refresh_centres=True, polygons=True)
    assert set(out) == set(plain) | {"polygons"} and all(torch.equal(out[k], plain[k]) for k in plain)
    P = out["polygons"]
    assert P["trajectories"] == [0, 1] and len(P["last"]) == 2
    for t, g in enumerate(graphs):
        X = tt(g[0], DEV)
        from graingraphnn_amd import GrainRollout
        alone = GrainRollout(R, Cm, X, tt(g[1], DEV), tt(g[2], DEV), 6, use_graph=True, refresh_centres=True)
        alone.enable_polygons(capacity=2)
        alone.run(2)
        for k in (0, 2):
            a, u = record(alone, k), P["at"](layer=k, traj=t)
            assert u["layers"] == 2
            assert_same_record(a, {key: u[key].cpu().numpy() for key in a if key != "layer"}, (t, k))
        assert torch.equal(P["last"][t]["xy_sorted"], alone.polygons()["xy_sorted"])


@pytest.mark.gpu
@torch.no_grad()
def test_folded_domain_against_the_restatement():
    """graph_120 folded by 3, one step: vertices and centres in the global frame (the fold belongs to x_grain)."""
    from graingraphnn_amd import GrainRollout
    from helpers import oracle
    x, ei, ea = load_graph("120")
    oX, oEA = tt(x), tt(ea)
    off, _ = oracle.scale_feature_patchs(3.0, oX, oEA)
    X = {k: v.clone().to(DEV) for k, v in oX.items()}
    R, Cm = product_models(0, 1.0, DEV)
    ro = GrainRollout(R, Cm, X, tt(ei, DEV), {k: v.clone().to(DEV) for k, v in oEA.items()}, 6, refresh_centres=True,
                      domain_factor=3.0, domain_offset=off)
    ro.enable_polygons(capacity=1)
    ro.step()
    got = record(ro)
    rowptr, col, kw, r = restated(ro)
    assert kw["domain_factor"] == 3.0 and kw["domain_offset"] is not None and got["layer"] == 1
    assert_equals_restatement(got, r, "folded x3")
    assert got["sides"].min() >= 3 and (got["area"] > 0).all()
    # x_grain carries the folded centre of the same polygon (test.py:558-559)
    folded = (got["centre"].astype(np.float64) * 3.0) % 1.0
    diff = np.abs(folded - X["grain"][:, :2].cpu().numpy())
    assert np.minimum(diff, 1 - diff).max() < 1e-5
    # the unfolded polygons tile the unit domain
    assert abs(float(got["area"].astype(np.float64).sum()) - 1.0) < 1e-4


@pytest.mark.gpu
@torch.no_grad()
def test_capacity_and_recapture():
    """polygons() raises once a layer went beyond the capacity; enabling after graphs were captured captures them again
    (the replays record); the default capacity is enable_qoi's and otherwise required."""
    ro, X = cfg1_rollout(polygons=None, use_graph=True)
    with pytest.raises(_lib.GGNNError, match="capacity"):
        ro.enable_polygons()
    ro.step()
    captured = ro._graphs
    assert captured
    ro.enable_polygons(capacity=2)
    assert ro._graphs is None
    first = record(ro)
    assert first["layer"] == 0
    assert_same_record(first, direct(ro), "layer 0 is the state at enabling")
    ro.step()
    ro.step()
    assert ro.polygons()["layers"] == 2 and ro._graphs
    assert_same_record(record(ro), direct(ro), "the re-captured graph records")
    assert_same_record(record(ro, 0), first, "layer 0 stays")
    with pytest.raises(_lib.GGNNError):
        ro.polygons(layer=3)
    ro.step()
    with pytest.raises(_lib.GGNNError, match="room"):
        ro.polygons()
    rq, _ = cfg1_rollout(polygons=None)
    rq.enable_qoi(40.0, 0.08, 2.0, 50.0)
    rq.enable_polygons()
    assert rq._poly["capacity"] == rq._qoi["capacity"] == 20
