"""In-between layers of a rollout and its 3-D volume (ggnn_polygon_inputs, ggnn_interp_polygons, GrainRollout.enable_polygons(
positions=True) / interp_polygons / grain_volume / orientation_volume, graingraphnn_amd.vtkio) against the numpy restatement
of tests/interpcheck.py and the reference's own frames of --interp_frames 2 (tests/golden/make_golden_interp.py).

Against the REFERENCE the contract of test_polygons (cyclic sequence for grains whose smallest angular gap is at least 1e-3
rad, start vertex away from the seam, centres to the centre goldens' bar, coordinates within 2^-23 of a shifted one); the
test refuses to exclude more than 1 % of a state's grains, and on periodic pairs it skips the grains that hold a junction
which crossed a wall between the two layers (the blend takes the short way there: departure 2 of DESIGN.md 8i), at most 5 %.
Against the float32 RESTATEMENT joint_sorted, xy_sorted and centre bit for bit, the area within polycheck.area_bound."""
import ctypes

import numpy as np
import pytest
import torch

import interpcheck
import polycheck
import rastercheck
from helpers import EDGE_TYPES, etk, load_graph, product_models, tt
from graingraphnn_amd import _lib, vtkio
from test_polygons import (assert_contract, assert_equals_restatement, assert_same_record, cfg1_rollout, npz, record,
                           synthetic_rows)

GJ, JG, JJ = EDGE_TYPES
DEV = "cuda"
PAIRS = ("static", "mass3", "noflux")
COEFFS = (1 / 3, 2 / 3)                    # interp_frames = 2
MAX_EXCLUDED, MAX_CROSSED = 0.01, 0.05     # shares of a state's grains (conditions, not measurements)


def pair_case(pair):
    """(X_prev, X_cur, joint->grain list of prev, of cur, boundary, n_grain, max_y) of a pair of recorded layers."""
    if pair == "noflux":
        d, G = npz("noflux_40_seed1"), npz("interp_cfg1")
        ei = d["ei_" + etk(JG)]
        return d["scaled_x_joint"][:, :2], G["noflux__x_joint_b"], ei, ei, "noflux", d["x_grain"].shape[0], float(d["max_y"])
    g40 = npz("graph_40")
    ei = g40["ei_" + etk(JG)]
    if pair == "static":
        return g40["x_joint"][:, :2], npz("golden_cfg1_centres")["step1_x_joint"][:, :2], ei, ei, "periodic", 118, 1.0
    ev = npz("golden_cfg1_events")
    return g40["x_joint"][:, :2], ev["mass3__out_x_joint"][:, :2], ei, ev["mass3__out_ei_" + etk(JG)], "periodic", 118, 1.0


def golden_frame(pair, i):
    G = npz("interp_cfg1")
    tag = f"{pair}_{i + 1}"
    rp = G[tag + "__rowptr"]
    regions = [G[tag + "__regions"][rp[g]:rp[g + 1]] if rp[g + 1] > rp[g] else None for g in range(len(rp) - 1)]
    coors = [G[tag + "__coors"][rp[g]:rp[g + 1]] for g in range(len(rp) - 1)]
    return regions, coors, G[tag + "__center"].copy()


def job_table(pair, c):
    xp, xc, ei_p, ei_c, bc, n, max_y = pair_case(pair)
    rowptr, col = polycheck.table_of(ei_c if c > 0.5 else ei_p, n)
    return xp, xc, rowptr, col, bc, n, max_y


# ---- CPU: the restatement against the reference --------------------------------------------------------------------------

@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("i", (0, 1))
def test_restatement_reproduces_the_references_frames(pair, i):
    """Measured: no grain of any of the six frames is below the gap limit (smallest gaps 0.185 / 0.184 rad in
    `static`, 0.088 / 0.019 in `mass3`, 0.0019 / 0.0019 in `noflux`), and no junction of the two periodic pairs crossed a
    wall between its layers, so no grain is skipped; the worst coordinate difference is 2^-24."""
    c = COEFFS[i]
    xp, xc, rowptr, col, bc, n, max_y = job_table(pair, c)
    regions, coors, centre = golden_frame(pair, i)
    assert all((r is None) == (rowptr[g + 1] - rowptr[g] < 2) for g, r in enumerate(regions))
    crossed = set()
    if bc == "periodic":   # departure 2: the grains that hold a junction which crossed a wall are not the reference's
        moved = interpcheck.crossed_a_wall(xc, xp)
        crossed = {g for g in range(n) if moved[col[rowptr[g]:rowptr[g + 1]]].any()}
        print(pair, c, "grains with a wall-crossing junction:", len(crossed))
        assert len(crossed) <= MAX_CROSSED * n, (pair, c, sorted(crossed))
        for g in crossed:
            regions[g], centre[g] = None, np.nan
    for dtype in (np.float64, np.float32):
        r = interpcheck.restate_job(rowptr, col, xc, xp, c, bc, max_y, dtype=dtype)
        cls = polycheck.classify(rowptr, col, r["positions"], boundary=bc)
        told = cls["gap"][np.isfinite(cls["gap"])]
        print(pair, c, dtype.__name__, "smallest gap", float(told.min()), "below the limit", int((told < polycheck.GAP_MIN).sum()))
        assert_contract(r["joint_sorted"], r["xy_sorted"], r["centre"], rowptr, cls, regions, coors, centre,
                        f"{pair} c={c:.3f} {dtype.__name__}", max_excluded_share=MAX_EXCLUDED)
    if bc == "noflux":   # the boundary grain: 38 sides on the walls, clockwise
        p = r["xy_sorted"][rowptr[0]:rowptr[1]]
        on_wall = (p[:, 0] == 0) | (p[:, 0] == 1) | (p[:, 1] == 0) | (p[:, 1] == np.float32(max_y))
        assert len(p) == 38 and on_wall.all() and r["area"][0] < 0
        assert r["positions"].min() >= 0 and r["positions"][:, 0].max() <= 1 and r["positions"][:, 1].max() <= max_y


def test_the_contract_rejects_a_record_built_with_the_wrong_layers_table():
    """mass3 at c = 2/3 has the NEW lists: the record built with the old ones fails the comparison."""
    xp, xc, ei_p, ei_c, bc, n, max_y = pair_case("mass3")
    regions, _, _ = golden_frame("mass3", 1)
    good_t, bad_t = polycheck.table_of(ei_c, n), polycheck.table_of(ei_p, n)
    for (rowptr, col), ok in ((good_t, True), (bad_t, False)):
        r = interpcheck.restate_job(rowptr, col, xc, xp, COEFFS[1], bc, max_y)
        cls = polycheck.classify(rowptr, col, r["positions"], boundary=bc)
        c = polycheck.compare_with_reference(r["joint_sorted"], rowptr, regions, cls)
        assert (not c["cyclic_bad"]) == ok, (ok, c)
    assert len(c["cyclic_bad"]) > 10


# ---- CPU: the rule's pins ------------------------------------------------------------------------------------------------------

def same_numbers(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))   # (+0 == -0)


@pytest.mark.parametrize("pair", PAIRS)
def test_endpoints_are_the_layers_own_records(pair):
    xp, xc, ei_p, ei_c, bc, n, max_y = pair_case(pair)
    if pair == "noflux":   # states as the step's boundary launch leaves them (the structure itself holds 1e-17 on its walls)
        d = npz("noflux_40_seed1")
        s1, s2 = d["s1_x_joint"][:, :2], d["s2_x_joint"][:, :2]
        ends = ((1.0, s1, xp, d["s1_ei_" + etk(JG)], s1), (0.0, s2, s1, d["s1_ei_" + etk(JG)], s1),
                (1.0, s2, s1, d["s2_ei_" + etk(JG)], s2))
    else:
        ends = ((1.0, xc, xp, ei_c, xc), (0.0, xc, xp, ei_p, xp))
    for c, x_l, x_prev, ei, own in ends:
        rowptr, col = polycheck.table_of(ei, n)
        r = interpcheck.restate_job(rowptr, col, x_l, x_prev, c, bc, max_y)
        want = polycheck.restate(rowptr, col, own, boundary=bc)
        assert np.array_equal(r["joint_sorted"], want["joint_sorted"]), (pair, c)
        assert same_numbers(r["xy_sorted"], want["xy_sorted"]) and same_numbers(r["centre"], want["centre"]), (pair, c)


def test_first_minimum_ties_and_junctions_outside_the_box():
    """One boundary grain (grain 0) with six junctions, a second grain that holds the same ones; c = 1: the positions are
    layer L's."""
    max_y = 0.75
    x_l = np.array([[0.25, 0.25],     # x = y: the first (x -> 0)
                    [0.5, 0.25],      # 1 - x = 0.5 > y = 0.25 ... y wins: y -> 0
                    [0.5, 0.375],     # x = 1 - x = 0.5 > y = max_y - y = 0.375: the first of the two (y -> 0)
                    [-0.1, -0.2],     # outside: the negative distance that is lower (y -> 0), then x clamped
                    [1.3, 0.5],       # 1 - x = -0.3 (x -> 1)
                    [0.9, 0.9],       # max_y - y = -0.15 (y -> max_y)
                    [0.3, 0.3]], np.float32)   # not in the boundary grain's row: stays
    rowptr, col = np.array([0, 6, 13]), np.array([0, 1, 2, 3, 4, 5, 6, 5, 4, 3, 2, 1, 0])
    x_prev = np.full_like(x_l, 0.5)
    got = interpcheck.positions(rowptr, col, x_l, x_prev, 1.0, "noflux", max_y)
    want = np.array([[0, 0.25], [0.5, 0], [0.5, 0], [0, 0], [1, 0.5], [0.9, 0.75], [0.3, 0.3]], np.float32)
    assert np.array_equal(got, want)
    # a union: the first grain of every trajectory that has grains
    got = interpcheck.positions(rowptr, col, x_l, x_prev, 1.0, "noflux", max_y, traj_grain_off=[0, 0, 1, 2])
    assert np.array_equal(got[6], np.array([0, 0.3], np.float32)) and np.array_equal(got[:6], want[:6])
    # periodic jobs neither snap nor clamp (departure 1)
    inside = np.clip(x_l, 0.0, 0.99).astype(np.float32)
    assert np.array_equal(interpcheck.positions(rowptr, col, inside, x_prev, 1.0, "periodic", max_y), inside)


def test_a_periodic_junction_takes_the_short_way_across_a_wall():
    x_prev, x_l = np.array([[0.98, 0.5]], np.float32), np.array([[0.03, 0.5]], np.float32)
    for c, lo, hi in ((0.5, 0.004, 0.006), (0.25, 0.99, 0.995), (0.75, 0.016, 0.019)):
        v = interpcheck.blend(x_l, x_prev, c, "periodic")
        assert lo < v[0, 0] < hi and v[0, 1] == 0.5, (c, v)
    assert abs(interpcheck.blend(x_l, x_prev, 0.5, "noflux")[0, 0] - 0.505) < 1e-6   # (no seam without a period)
    # where no junction crossed a wall the blend is the reference's formula to the bit
    rs = np.random.RandomState(3)
    a, b = rs.uniform(0.3, 0.7, (50, 2)).astype(np.float32), rs.uniform(0.3, 0.7, (50, 2)).astype(np.float32)
    for c in COEFFS:
        ref = (c * torch.from_numpy(a) + (1 - c) * torch.from_numpy(b)).numpy()
        assert np.array_equal(interpcheck.blend(a, b, c, "periodic").view(np.int32), ref.view(np.int32))


def test_volume_order_is_the_scripts():
    assert interpcheck.volume_order([0, 1, 2], 2) == [("layer", 0), ("job", 1, 1 / 3), ("job", 1, 2 / 3), ("layer", 1),
                                                      ("job", 2, 1 / 3), ("job", 2, 2 / 3), ("layer", 2)]
    assert interpcheck.volume_order([0, 2], 1) == [("layer", 0), ("job", 2, 0.5), ("layer", 2)]


# ---- CPU: the file ---------------------------------------------------------------------------------------------------------------

def test_vtk_round_trip_header_and_byte_order(tmp_path):
    vol = (np.arange(3 * 4 * 5, dtype=np.float32) * 1.25 - 7).reshape(3, 4, 5)   # [nz, ny, nx], distinct values
    path = tmp_path / "seed0graph.vtk"
    size = vtkio.write_vtk(path, vol, (0.5, 0.5, 2.0))
    raw = path.read_bytes()
    assert size == len(raw)
    head, body = raw[:len(raw) - 4 * vol.size - 1], raw[len(raw) - 4 * vol.size - 1:-1]
    assert head.decode("ascii").split("\n") == [
        "# vtk DataFile Version 3.0", "grain structure", "BINARY", "DATASET STRUCTURED_POINTS", "DIMENSIONS 5 4 3",
        "SPACING 0.5 0.5 2.0", "ORIGIN 0.0 0.0 0.0", "POINT_DATA 60", "SCALARS theta_z float", "LOOKUP_TABLE default", ""]
    assert raw.endswith(b"\n")
    # big-endian float32, x fastest: the second value is the point (x = 1, y = 0, z = 0)
    assert body[:8] == np.array([vol[0, 0, 0], vol[0, 0, 1]], ">f4").tobytes()
    assert np.array_equal(np.frombuffer(body, ">f4"), vol.ravel())
    assert np.array_equal(np.frombuffer(body, ">f4"), np.transpose(vol, (2, 1, 0)).ravel(order="F"))   # pv_3Dview.py:188
    back = vtkio.read_vtk(path)
    assert back["volume"].dtype == np.float32 and np.array_equal(back["volume"], vol)
    assert back["spacing"] == (0.5, 0.5, 2.0) and back["origin"] == (0.0, 0.0, 0.0) and back["name"] == "theta_z"
    ids = torch.arange(24, dtype=torch.int32).reshape(2, 3, 4)   # an integer tensor is written as float32
    vtkio.write_vtk(path, ids, (1, 1, 1), name="grain")
    back = vtkio.read_vtk(path)
    assert back["name"] == "grain" and np.array_equal(back["volume"], ids.numpy().astype(np.float32))
    for bad in (dict(volume=vol[0]), dict(spacing=(1, 1)), dict(spacing=(1, 0, 1)), dict(name="two words")):
        with pytest.raises(ValueError):
            vtkio.write_vtk(path, **{**dict(volume=vol, spacing=(1, 1, 1)), **bad})
    path.write_bytes(raw[:-20])
    with pytest.raises(ValueError):
        vtkio.read_vtk(path)


# ---- CPU: the entry points ----------------------------------------------------------------------------------------------------

def test_entry_points_validate_on_the_host():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.PolygonInputsArgs) == 6 * 8 + 4 * 8 + 8 and ctypes.sizeof(_lib.InterpArgs) == 12 * 8 + 7 * 8 + 8
    assert _lib.GGNN_INTERP_MAX_JOBS == 256 and _lib.GGNN_ABI_VERSION == 26
    buf = (ctypes.c_float * 64)()                 # (host memory: refused before anything would be launched)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.ggnn_polygon_inputs(None, None) == -1 and lib.ggnn_interp_polygons(None, None) == -1
    assert lib.ggnn_polygon_inputs(ctypes.byref(_lib.PolygonInputsArgs()), None) == -1
    assert lib.ggnn_interp_polygons(ctypes.byref(_lib.InterpArgs()), None) == -1

    def inputs(**kw):
        A = _lib.PolygonInputsArgs(p, p, None, p, p, None, 4, 2, 9, 0, 1.0)
        for k, v in kw.items():
            setattr(A, k, v)
        return ctypes.byref(A)
    for bad in (dict(col=None), dict(x_joint=None), dict(col_out=None), dict(joint_xy=None), dict(n_joint=0), dict(ldx_joint=1),
                dict(E_cap=-1), dict(capacity=-1), dict(capacity=2 ** 31), dict(domain_factor=0.5), dict(domain_factor=float("nan"))):
        assert lib.ggnn_polygon_inputs(inputs(**bad), None) == -1, bad

    def interp(job_layers=(1,), job_coeffs=(0.5,), **kw):
        hl, hc = (ctypes.c_int32 * len(job_layers))(*job_layers), (ctypes.c_double * len(job_coeffs))(*job_coeffs)
        A = _lib.InterpArgs(p, p, p, None, ctypes.cast(hl, ctypes.c_void_p), ctypes.cast(hc, ctypes.c_void_p), p, p, p, p, p, p,
                            4, 3, 9, 2, 2, 1, len(job_layers), 1.0, _lib.BC_PERIODIC)
        for k, v in kw.items():
            setattr(A, k, v)
        return lib.ggnn_interp_polygons(ctypes.byref(A), None)
    for bad in (dict(rowptr=None), dict(col=None), dict(joint_xy=None), dict(job_layer=None), dict(job_coeff=None), dict(work=None),
                dict(rowptr_out=None), dict(joint_sorted=None), dict(xy_sorted=None), dict(centre=None), dict(area=None),
                dict(boundary=7), dict(n_joint=0), dict(n_grain=0), dict(E_cap=-1), dict(capacity=-1), dict(layers=0),
                dict(layers=3), dict(n_jobs=0), dict(n_traj=2), dict(traj_grain_off=p, n_traj=0),
                dict(boundary=_lib.BC_NOFLUX, max_y=0.0), dict(boundary=_lib.BC_NOFLUX, max_y=float("nan"))):
        assert interp(**bad) == -1, bad
    for layers, coeffs in (((0,), (0.5,)), ((3,), (0.5,)), ((-1,), (0.5,)), ((1,), (-1e-9,)), ((1,), (1.0000001,)),
                           ((1,), (float("nan"),)), ((1, 2, 0), (0.1, 0.2, 0.3)), ((1,) * 257, (0.5,) * 257)):
        assert interp(layers, coeffs) == -1, (layers[:3], coeffs[:3])


def test_rollout_refuses_in_between_layers_without_positions():
    from graingraphnn_amd import GrainRollout
    ro = object.__new__(GrainRollout)
    ro._poly = None
    for call in (lambda: ro.interp_polygons(1, 0.5), lambda: ro.grain_volume((8, 8), interp_frames=1),
                 lambda: ro.grain_volume((8, 8))):
        with pytest.raises(_lib.GGNNError, match="enable_polygons"):
            call()
    ro._poly = {"inputs": None}
    with pytest.raises(_lib.GGNNError, match="positions=True"):
        ro.grain_volume((8, 8), interp_frames=2)
    with pytest.raises(_lib.GGNNError, match="negative"):
        ro.grain_volume((8, 8), interp_frames=-1)


def test_orientation_table_is_formed_in_float64_and_rounded_once():
    from graingraphnn_amd import GrainRollout
    theta = np.concatenate([[0.0], np.random.RandomState(1).uniform(0, np.pi / 2, 7)])
    ids = torch.tensor([[[0, 1, 2], [7, 3, 0]]], dtype=torch.int32)
    got = GrainRollout.orientation_volume(ids, theta)
    want = (theta[ids.numpy()] / np.pi * 180).astype(np.float32)      # pv_3Dview.py:178, rounded to fp32
    assert got.dtype == torch.float32 and got.shape == ids.shape and np.array_equal(got.numpy(), want)
    with pytest.raises(_lib.GGNNError):
        GrainRollout.orientation_volume(ids, theta[:7])


# ---- GPU: the kernels alone ---------------------------------------------------------------------------------------------

JOBS = ((1, 0.0), (1, 0.25), (1, 1 / 3), (1, 0.5), (1, 2 / 3), (1, 0.9), (1, 1.0))   # both topologies, both endpoints
UNION3 = (0, 4, 7)                                  # + n_grain: first grains with 0, 15 and 63 junctions (test_polygons.ROWS)


def fold(xy, factor):
    """Global positions -> (the state's columns, domain_offset) as scale_feature_patchs folds them."""
    if factor == 1.0:
        return xy.astype(np.float32), None
    scaled = xy.astype(np.float32) * np.float32(factor)
    off = np.floor(scaled).astype(np.float32)
    return scaled - off, off


def unfold(x, off, factor):
    """The expression ggnn_grain_polygons unwraps from, in float32."""
    x = np.asarray(x, np.float32)[:, :2]
    return x if factor == 1.0 else ((x + off).astype(np.float32) / np.float32(factor)).astype(np.float32)


def two_synthetic_layers(boundary, factor):
    """Layer 0 = test_polygons.synthetic_rows; layer 1 = its junctions displaced (periodic: wrapped, so junctions near a
    wall cross it) with another table: the list's columns shuffled again and the last grain's entries dropped.
    -> [(x_joint, list, domain_offset)] * 2, n_grain"""
    xa, ei_a, n_grain, off_a = synthetic_rows(boundary, factor)
    rs = np.random.RandomState(23)
    ga = unfold(xa, off_a, factor).astype(np.float64)
    gb = ga + rs.normal(0.0, 0.012, ga.shape)
    if boundary == "periodic":
        gb -= np.floor(gb)
    xb = xa.copy()
    xb[:, :2], off_b = fold(gb, factor)
    keep = np.flatnonzero(ei_a[1] != n_grain - 1)
    ei_b = ei_a[:, keep[rs.permutation(len(keep))]]
    return [(xa, ei_a, off_a), (xb, ei_b, off_b)], n_grain


def record_layers(be, layers, n_grain, boundary, factor, traj=None):
    """ggnn_polygon_inputs + ggnn_grain_polygons per layer, on one layer word.  -> (arena, inputs, numpy read-backs)."""
    from types import SimpleNamespace
    n_joint, E = layers[0][0].shape[0], max(l[1].shape[1] for l in layers)
    arena = be.polygon_arena(n_grain, E, len(layers) - 1, DEV)
    inputs = be.polygon_inputs_arena(n_joint, E, len(layers) - 1, DEV)
    word, words = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    cols = []
    for k, (xj, ei, off) in enumerate(layers):
        csr = be.build_csr(torch.from_numpy(ei).to(DEV), n_joint, n_grain)
        col = torch.full((E,), 2 ** 31 - 1, dtype=torch.int32, device=DEV)   # (a shrunken table leaves stale entries behind)
        col[:csr.col.numel()] = csr.col
        cols.append(csr.col.cpu().numpy())
        table = SimpleNamespace(rowptr=csr.rowptr, col=col)
        X, O = torch.from_numpy(xj).to(DEV), None if off is None else torch.from_numpy(off).to(DEV)
        be.polygon_inputs(table, X, inputs, factor, O, layer_in=word if k else None)
        be.grain_polygons(table, X, arena, factor, O, boundary=boundary, traj_grain_off=traj, layer_in=word if k else None,
                          layer_out=word, sync_word=words[:1], flags=words[1:])
        assert int(word) == k and words.tolist() == [0, 0]
    back = {"rowptr": arena["rowptr"].cpu().numpy(), "col": inputs["col"].cpu().numpy(), "xy": inputs["joint_xy"].cpu().numpy()}
    for k, (xj, ei, off) in enumerate(layers):   # the recorder: the table's columns as they are, the global frame's expression
        e = ei.shape[1]
        assert back["rowptr"][k, -1] == e and np.array_equal(back["col"][k, :e], cols[k][:e]) and (back["col"][k, e:] == 2 ** 31 - 1).all()
        assert np.array_equal(back["xy"][k].view(np.int32), unfold(xj, off, factor).view(np.int32)), k
    return arena, inputs, back


def job_restated(back, L, c, boundary, max_y, traj):
    T = L if c > 0.5 else L - 1
    rowptr = back["rowptr"][T]
    return rowptr, interpcheck.restate_job(rowptr, back["col"][T][:rowptr[-1]], back["xy"][L], back["xy"][L - 1], c, boundary, max_y,
                                           traj)


def job_numpy(out, i):
    got = {k: v[i].cpu().numpy() for k, v in out.items()}
    E = int(got["rowptr"][-1])
    got["joint_sorted"], got["xy_sorted"] = got["joint_sorted"][:E], got["xy_sorted"][:E]
    return got


def assert_jobs_equal_restatement(out, back, jobs, boundary, max_y, traj, what):
    for i, (L, c) in enumerate(jobs):
        rowptr, r = job_restated(back, L, c, boundary, max_y, traj)
        got = job_numpy(out, i)
        assert np.array_equal(got["rowptr"], rowptr), (what, i)
        assert_equals_restatement(got, r, f"{what} job {i} c={c:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("boundary,factor,union", [("periodic", 1.0, False), ("periodic", 3.0, False), ("noflux", 1.0, True),
                                                   ("noflux", 3.0, False)])
def test_kernel_against_the_restatement_on_synthetic_layers(boundary, factor, union):
    """Seven jobs in one launch over two layers with different tables: rows of 0..3, 15 / 16 / 17 and 63 / 64 / 65 junctions
    and the common 3..12, junctions that cross the periodic walls, a no-flux union of three trajectories whose boundary
    grains have 0, 15 and 63 junctions (the group's path and the wave's)."""
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    layers, n_grain = two_synthetic_layers(boundary, factor)
    traj = np.asarray(UNION3 + (n_grain,), np.int64) if union else None
    traj_dev = None if traj is None else torch.from_numpy(traj).to(DEV)
    max_y = 1.0 if boundary == "periodic" else 0.875
    arena, inputs, back = record_layers(be, layers, n_grain, boundary, factor, traj_dev)
    assert back["rowptr"][0, -1] > back["rowptr"][1, -1] and not np.array_equal(back["col"][0], back["col"][1])
    crossed = interpcheck.crossed_a_wall(back["xy"][1], back["xy"][0])
    assert crossed.any() == (boundary == "periodic")
    out = be.interp_polygons(arena, inputs, JOBS, 1, boundary, max_y, traj_dev)
    assert_jobs_equal_restatement(out, back, JOBS, boundary, max_y, traj, f"{boundary} x{factor:g}")
    if boundary == "periodic":   # the endpoints are the layers' own records, and a crossing junction took the short way
        for i, k in ((0, 0), (len(JOBS) - 1, 1)):
            got, own = job_numpy(out, i), job_numpy(arena, k)
            assert np.array_equal(got["joint_sorted"], own["joint_sorted"]) and np.array_equal(got["rowptr"], own["rowptr"])
            assert same_numbers(got["xy_sorted"], own["xy_sorted"]) and np.array_equal(got["centre"], own["centre"]), i
        mid = interpcheck.blend(back["xy"][1], back["xy"][0], 0.5, boundary)
        far = np.abs(mid - 0.5 * (back["xy"][1].astype(np.float64) + back["xy"][0]))
        assert (far[crossed].max(axis=1) > 0.4).all() and far[~crossed].max() < 1e-6
    else:   # every boundary grain's junctions lie on a wall, every junction in the box
        _, r = job_restated(back, 1, 2 / 3, boundary, max_y, traj)
        on_wall = lambda p: (p[:, 0] == 0) | (p[:, 0] == 1) | (p[:, 1] == 0) | (p[:, 1] == np.float32(max_y))
        rowptr = back["rowptr"][1]
        for g in polycheck.boundary_grains(n_grain, boundary, traj):
            assert on_wall(job_numpy(out, 4)["xy_sorted"][rowptr[g]:rowptr[g + 1]]).all(), g
        assert not on_wall(r["positions"]).all() and r["positions"].min() >= 0 and r["positions"][:, 1].max() <= max_y


@pytest.mark.gpu
def test_kernel_on_the_noflux_fixture_with_ties_and_junctions_outside_the_box():
    """The 40 um no-flux structure (a boundary grain of 38 sides: the wave's path) and its displaced copy, in which four
    junctions of the boundary grain are put where the first minimum has to decide and outside the box."""
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    xp, xc, ei, _, bc, n, max_y = pair_case("noflux")
    rowptr, col = polycheck.table_of(ei, n)
    assert rowptr[1] - rowptr[0] == 38 and max_y == 1.0
    xc = xc.copy()
    pins = {int(col[0]): (0.25, 0.25), int(col[5]): (0.5, 0.5), int(col[11]): (-0.1, -0.2), int(col[17]): (1.3, 0.5)}
    for j, v in pins.items():
        xc[j] = v
    layers = [(np.ascontiguousarray(xp), ei, None), (xc, ei, None)]
    arena, inputs, back = record_layers(be, layers, n, bc, 1.0)
    out = be.interp_polygons(arena, inputs, JOBS, 1, bc, max_y)
    assert_jobs_equal_restatement(out, back, JOBS, bc, max_y, None, "noflux fixture")
    _, last = job_restated(back, 1, 1.0, bc, max_y, None)
    want = {(0.25, 0.25): (0, 0.25), (0.5, 0.5): (0, 0.5), (-0.1, -0.2): (0, 0), (1.3, 0.5): (1, 0.5)}
    for j, v in pins.items():
        assert tuple(last["positions"][j]) == want[v], (j, v)
    sides = np.diff(rowptr)
    for i in range(len(JOBS)):
        got = job_numpy(out, i)
        assert got["area"][0] < 0 and (got["area"][1:][sides[1:] >= 3] != 0).all()


@pytest.mark.gpu
def test_kernels_clamp_whatever_the_tables_hold():
    """Row pointers and columns outside the arrays, NaN and infinite positions, in the recorder's arrays of both layers:
    the launches address nothing outside their arrays -- the guard words round every output and the workspace stay -- and
    copy the row pointers as they are."""
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    for boundary in ("periodic", "noflux"):
        layers, n_grain = two_synthetic_layers(boundary, 1.0)
        arena, inputs, back = record_layers(be, layers, n_grain, boundary, 1.0)
        E, n_joint = inputs["col"].size(1), inputs["joint_xy"].size(1)
        rs = np.random.RandomState(5)
        for k in (0, 1):
            wild = back["rowptr"][k].copy()
            wild[[3, 9, 20, -1]] = [-4, E + 1000, -2 ** 31, 2 ** 31 - 1]
            arena["rowptr"][k] = torch.from_numpy(wild).to(DEV)
            col = back["col"][k].copy()
            col[rs.randint(0, E, 40)] = rs.choice([-1, -2 ** 31, n_joint, 2 ** 31 - 1, 10 ** 6], 40)
            inputs["col"][k] = torch.from_numpy(col).to(DEV)
            xy = back["xy"][k].copy()
            xy[rs.randint(0, n_joint, 12)] = rs.choice([np.nan, np.inf, -np.inf, 3e38, -1e30], (12, 2))
            inputs["joint_xy"][k] = torch.from_numpy(xy).to(DEV)
        wild = arena["rowptr"].cpu().numpy()
        nj = len(JOBS)
        sizes = {"rowptr": (nj, n_grain + 1), "joint_sorted": (nj, E), "xy_sorted": (nj, E, 2), "centre": (nj, n_grain, 2),
                 "area": (nj, n_grain)}
        guarded, out = {}, {}
        for name, shape in sizes.items():
            dtype = torch.int32 if name in ("rowptr", "joint_sorted") else torch.float32
            n = int(np.prod(shape))
            guarded[name] = torch.full((n + 128,), -9, dtype=dtype, device=DEV)
            out[name] = guarded[name][64:64 + n].view(shape)
        be.interp_polygons(arena, inputs, JOBS, 1, boundary, 1.0, out=out)
        torch.cuda.synchronize()
        for name, g in guarded.items():
            assert bool((g[:64] == -9).all()) and bool((g[-64:] == -9).all()), (boundary, name)
        for i, (L, c) in enumerate(JOBS):
            assert np.array_equal(out["rowptr"][i].cpu().numpy(), wild[L if c > 0.5 else L - 1]), (boundary, i)
        assert bool(((out["joint_sorted"] == -9) | ((out["joint_sorted"] >= 0) & (out["joint_sorted"] < n_joint))).all())


# ---- GPU: the recorder in rollouts --------------------------------------------------------------------------------------

def positions_on(ro, capacity):
    ro.enable_polygons(capacity=capacity, positions=True)
    return ro


def state_inputs(ro):
    """(col of the live table, junctions in the global frame) of the rollout's state as it is."""
    csr = ro.graph.csr_full[JG]
    off = None if ro.domain_offset is None else ro.domain_offset.cpu().numpy()
    return (csr.col[:int(csr.rowptr[-1])].cpu().numpy(), unfold(ro.x["joint"].cpu().numpy(), off, float(ro.domain_factor)))


def recorded_inputs(ro, layer=None, traj=None):
    p = ro.polygons(layer, traj)
    return p["col"].cpu().numpy().copy(), p["joint_xy"].cpu().numpy().copy()


def assert_inputs(a, b, what):
    assert np.array_equal(a[0], b[0]), (what, "col")
    assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32)), (what, "joint_xy")


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["joint", "overlapped"])
@torch.no_grad()
def test_recorder_in_eager_steps_and_graph_replays(plan):
    """col and joint_xy of every layer are the table and the state read back after that step; run(6) as two replays of a
    3-step hipGraph records the same rows; the final state is the state of a rollout that records polygons alone, and of
    one that records nothing."""
    kw = dict(joint_launches=plan == "joint", concurrent=True)
    eager, Xe = cfg1_rollout(polygons=None, use_graph=False, **kw)
    positions_on(eager, 6)
    by_hand = [state_inputs(eager)]
    assert_inputs(recorded_inputs(eager), by_hand[0], "layer 0 at enabling")
    for k in range(1, 7):
        eager.step()
        by_hand.append(state_inputs(eager))
        assert_inputs(recorded_inputs(eager), by_hand[k], (plan, "eager", k))
    graphed, Xg = cfg1_rollout(polygons=None, use_graph=True, **kw)
    positions_on(graphed, 6)
    graphed.RUN_UNROLL = 3
    graphed.run(6)
    plain, Xp = cfg1_rollout(polygons=6, use_graph=True, **kw)
    plain.RUN_UNROLL = 3
    plain.run(6)
    assert "col" not in plain.polygons() and plain._poly["inputs"] is None
    for k in range(7):
        assert_inputs(recorded_inputs(graphed, k), by_hand[k], (plan, "graph", k))
        assert_same_record(record(graphed, k), record(plain, k), (plan, k))
        assert_same_record(record(eager, k), record(plain, k), (plan, k))
    assert not np.array_equal(by_hand[0][1], by_hand[6][1])
    off, Xo = cfg1_rollout(polygons=None, use_graph=True, **kw)
    off.RUN_UNROLL = 3
    off.run(6)
    for nt in Xe:
        assert torch.equal(Xe[nt], Xo[nt]) and torch.equal(Xg[nt], Xo[nt]) and torch.equal(Xp[nt], Xo[nt]), nt
    for et in EDGE_TYPES:
        assert torch.equal(graphed.edge_attr_dict()[et], off.edge_attr_dict()[et]), et


@pytest.mark.gpu
@torch.no_grad()
def test_off_means_off():
    """Without positions=True a step calls the entry points it called before; with it, ggnn_polygon_inputs once more, right
    in front of ggnn_grain_polygons."""
    from graingraphnn_amd.backend import default_backend
    from test_qoi import _CountingLib
    be = default_backend()
    calls = {}
    for mode in ("none", "polygons", "positions"):
        ro, _ = cfg1_rollout(polygons=None, use_graph=False)
        if mode != "none":
            ro.enable_polygons(capacity=4, positions=mode == "positions")
        ro.step()
        lib = be.lib
        be.lib = counting = _CountingLib(lib)
        try:
            ro.step()
        finally:
            be.lib = lib
        calls[mode] = counting.calls
    assert "ggnn_polygon_inputs" not in calls["none"] + calls["polygons"]
    assert [c for c in calls["polygons"] if c != "ggnn_grain_polygons"] == calls["none"]
    at = calls["positions"].index("ggnn_polygon_inputs")
    assert calls["positions"][at + 1] == "ggnn_grain_polygons" and calls["positions"].count("ggnn_polygon_inputs") == 1
    assert calls["positions"][:at] + calls["positions"][at + 1:] == calls["polygons"]


@pytest.mark.gpu
@torch.no_grad()
def test_recorder_with_events_step_by_step_and_speculative():
    """The seeded 40 um trajectory whose steps 3 and 4 eliminate 22 and 75 grains (test_polygons): every layer's inputs are
    that step's table and state; run_events() -- speculative blocks, voided steps written again -- records the same; the
    in-between layers across the eventful step have the old lists at 1/3 and the new ones at 2/3."""
    mask = {"grain": np.ones((118, 1)), "joint": np.ones((236, 1))}
    kw = dict(use_graph=True, joint_launches=False, concurrent=True)
    ra, Xa = cfg1_rollout(polygons=None, **kw)
    rb, Xb = cfg1_rollout(polygons=None, **kw)
    for ro in (ra, rb):
        positions_on(ro, 6)
        ro.enable_events(mask, 1e-4, 0.6)
    events = []
    for k in range(1, 6):
        events.append(len(ra.step_events()[1]))
        assert_inputs(recorded_inputs(ra), state_inputs(ra), ("step_events", k))
    assert events[:4] == [0, 0, 22, 75]
    for n in (3, 2):
        rb.run_events(n)
    for nt in Xa:
        assert torch.equal(Xa[nt], Xb[nt]), nt
    for k in range(6):
        assert_inputs(recorded_inputs(ra, k), recorded_inputs(rb, k), ("run_events", k))
        assert_same_record(record(ra, k), record(rb, k), ("run_events", k))
    for c, T in ((1 / 3, 2), (2 / 3, 3)):
        got = ra.interp_polygons(3, c)
        own = record(ra, T)
        assert got["layer"] == T and np.array_equal(got["rowptr"].cpu().numpy(), own["rowptr"])
        rowptr, r = job_restated({"rowptr": {T: own["rowptr"]}, "col": {T: recorded_inputs(ra, T)[0]},
                                  "xy": {3: recorded_inputs(ra, 3)[1], 2: recorded_inputs(ra, 2)[1]}}, 3, c, "periodic", 1.0, None)
        assert_equals_restatement({k: got[k].cpu().numpy() for k in ("joint_sorted", "xy_sorted", "centre", "area")}, r,
                                  f"across the eventful step c={c:.3f}")
    assert (record(ra, 2)["sides"] == 0).sum() == 0 and (record(ra, 3)["sides"] == 0).sum() == 22


@pytest.mark.gpu
@torch.no_grad()
def test_recorder_in_a_union_per_trajectory_and_through_rollout_trajectories():
    """A periodic union of two trajectories: polygons(traj=t) hands out the trajectory's own junctions and local columns,
    equal to its own rollout's; dist.rollout_trajectories(polygons=True, positions=True) hands the option through."""
    from graingraphnn_amd import GrainRollout, dist
    from test_ensemble_events import cfg1
    graphs = [cfg1(), cfg1("perturbed", 1000, 1e-3)]
    R, Cm = product_models(10020, 1.0, DEV)
    plain = dist.rollout_trajectories(R, Cm, graphs, 6, 2, refresh_centres=True, polygons=True)
    out = dist.rollout_trajectories(R, Cm, graphs, 6, 2, refresh_centres=True, polygons=True, positions=True)
    assert all(torch.equal(out[k], plain[k]) for k in plain if k != "polygons")
    P = out["polygons"]
    assert set(P) == set(plain["polygons"]) | {"interp", "volume"}
    for t, g in enumerate(graphs):
        alone = GrainRollout(R, Cm, tt(g[0], DEV), tt(g[1], DEV), tt(g[2], DEV), 6, use_graph=True, refresh_centres=True)
        positions_on(alone, 2)
        alone.run(2)
        for k in range(3):
            u = P["at"](layer=k, traj=t)
            assert u["joint_xy"].shape == (236, 2) and int(u["col"].min()) >= 0 and int(u["col"].max()) < 236
            assert_inputs(recorded_inputs(alone, k), (u["col"].cpu().numpy(), u["joint_xy"].cpu().numpy()), (t, k))
        a, u = alone.interp_polygons(2, 0.5), P["interp"](2, 0.5, traj=t)
        for key in ("rowptr", "joint_sorted", "xy_sorted", "centre", "area", "sides"):
            assert torch.equal(a[key], u[key]), (t, key)
        assert torch.equal(alone.grain_volume((41, 41), 1), P["volume"]((41, 41), 1, traj=t)), t


@pytest.mark.gpu
@torch.no_grad()
def test_recorder_in_a_folded_domain_and_its_capacity():
    """graph_120 folded by 3: joint_xy is the global frame's; a layer beyond the capacity writes nothing (the guard rows
    behind the arrays stay) and polygons() raises as it does for the polygon rows."""
    from graingraphnn_amd import GrainRollout
    from helpers import oracle
    x, ei, ea = load_graph("120")
    oX, oEA = tt(x), tt(ea)
    off, _ = oracle.scale_feature_patchs(3.0, oX, oEA)
    X = {k: v.clone().to(DEV) for k, v in oX.items()}
    R, Cm = product_models(0, 1.0, DEV)
    ro = GrainRollout(R, Cm, X, tt(ei, DEV), {k: v.clone().to(DEV) for k, v in oEA.items()}, 6, refresh_centres=True,
                      domain_factor=3.0, domain_offset=off)
    positions_on(ro, 1)
    big = ro.be.polygon_inputs_arena(X["joint"].size(0), ro._poly["inputs"]["col"].size(1), 2, DEV)
    for name, v in big.items():   # the same rows with a guard row behind them
        v.fill_(-7)
        v[:2] = ro._poly["inputs"][name]
        ro._poly["inputs"][name] = v[:2]
    ro.step()
    got = recorded_inputs(ro)
    assert_inputs(got, state_inputs(ro), "folded x3")
    assert not np.array_equal(got[1], X["joint"][:, :2].cpu().numpy())
    mid = ro.interp_polygons(1, 0.5)
    assert abs(float(mid["area"].double().sum()) - 1.0) < 1e-4   # the in-between polygons tile the unit domain
    kept = {k: v.clone() for k, v in big.items()}
    ro.step()
    for k, v in big.items():
        assert torch.equal(v, kept[k]) and bool((v[2] == -7).all()), k
    with pytest.raises(_lib.GGNNError, match="room"):
        ro.polygons()
    with pytest.raises(_lib.GGNNError, match="room"):
        ro.grain_volume((32, 32), interp_frames=1)


# ---- GPU: through the rollout ---------------------------------------------------------------------------------------------

def back_of(ro, layers):
    return {"rowptr": {k: record(ro, k)["rowptr"] for k in layers}, "col": {k: recorded_inputs(ro, k)[0] for k in layers},
            "xy": {k: recorded_inputs(ro, k)[1] for k in layers}}


def volume_restated(ro, back, size, interp_frames, layers, boundary, max_y=1.0, **kw):
    images = []
    for item in interpcheck.volume_order(layers, interp_frames):
        if item[0] == "layer":
            p = record(ro, item[1])
            images.append(rastercheck.grain_image(p["rowptr"], p["xy_sorted"], size, boundary, **kw))
        else:
            rowptr, r = job_restated(back, item[1], item[2], boundary, max_y, None)
            images.append(rastercheck.grain_image(rowptr, r["xy_sorted"], size, boundary, **kw))
    return np.stack(images)


@pytest.mark.gpu
@torch.no_grad()
def test_volume_through_the_rollout():
    """Three steps of the 40 um fixture: the endpoints are the layers' own records; grain_volume(interp_frames=2) is, pixel
    for pixel, the restated jobs and the recorded layers in test.py's order; interp_frames=0 is grain_images;
    orientation_volume is the float64 expression rounded once; and a rollout whose volumes were taken between its steps
    ends bit-equal to one that took none."""
    size = (61, 61)
    ro, X = cfg1_rollout(polygons=None, use_graph=True)
    quiet, Xq = cfg1_rollout(polygons=None, use_graph=True)
    positions_on(ro, 3)
    for k in range(1, 4):
        ro.step()
        quiet.step()
        part = ro.grain_volume(size, interp_frames=2)
        assert part.shape == (1 + 3 * k, 61, 61) and part.dtype == torch.int32
    for nt in X:
        assert torch.equal(X[nt], Xq[nt]), nt
    for L in (1, 2, 3):
        for c, k in ((1.0, L), (0.0, L - 1)):
            got, own = ro.interp_polygons(L, c), ro.polygons(k)
            assert got["layer"] == k
            for key in ("rowptr", "joint_sorted", "centre", "sides"):
                assert torch.equal(got[key], own[key]), (L, c, key)
            assert same_numbers(got["xy_sorted"].cpu().numpy(), own["xy_sorted"].cpu().numpy()), (L, c)
    back = back_of(ro, range(4))
    vol = ro.grain_volume(size, interp_frames=2)
    want = volume_restated(ro, back, size, 2, range(4), "periodic")
    assert vol.shape == (10, 61, 61) and np.array_equal(vol.cpu().numpy(), want)
    assert len({v.tobytes() for v in want}) == 10   # ten different images
    assert torch.equal(part, vol)
    some = ro.grain_volume(size, interp_frames=1, layers=[0, 2])
    assert np.array_equal(some.cpu().numpy(), volume_restated(ro, back, size, 1, [0, 2], "periodic"))
    assert torch.equal(ro.grain_volume(size), ro.grain_images(size))
    assert torch.equal(ro.grain_volume(size, 0, layers=[3, 1]), ro.grain_images(size, [3, 1]))
    into = torch.full((10, 61, 61), -1, dtype=torch.int32, device=DEV)
    assert ro.grain_volume(size, 2, out=into) is into and torch.equal(into, vol)
    theta = np.concatenate([[0.0], np.random.RandomState(4).uniform(0, np.pi / 2, 118)])
    deg = ro.orientation_volume(vol, theta)
    assert deg.dtype == torch.float32 and deg.shape == vol.shape and deg.is_cuda
    assert np.array_equal(deg.cpu().numpy(), (theta[want] / np.pi * 180).astype(np.float32))
    for bad in (lambda: ro.interp_polygons(0, 0.5), lambda: ro.interp_polygons(4, 0.5), lambda: ro.interp_polygons(1, 1.5),
                lambda: ro.interp_polygons(1, float("nan")), lambda: ro.grain_volume(size, 1, layers=[5])):
        with pytest.raises(_lib.GGNNError):
            bad()
    plain, _ = cfg1_rollout(polygons=1)
    plain.step()
    with pytest.raises(_lib.GGNNError, match="positions=True"):
        plain.grain_volume(size, interp_frames=1)
    with pytest.raises(_lib.GGNNError, match="positions=True"):
        plain.interp_polygons(1, 0.5)


@pytest.mark.gpu
@torch.no_grad()
def test_noflux_volume_through_the_rollout():
    """Two steps of the 40 um no-flux fixture: between stepped layers the endpoints are the layers' own records (layer 0, the
    structure itself, holds 1e-17 where its wall junctions should hold 0, so its endpoint is not asked); the volume with
    corner grains is the restated one, the boundary grain's junctions on the walls in every in-between layer."""
    from test_noflux import fixture
    from test_noflux_ensemble import F40, nf_graph, nf_rollout
    d = fixture(F40)
    ro, X, _ = nf_rollout(d, [nf_graph(d)], False, events=False, union=False)
    positions_on(ro, 2)
    ro.step()
    ro.step()
    for c, k in ((1.0, 2), (0.0, 1)):
        got, own = ro.interp_polygons(2, c), ro.polygons(k)
        for key in ("rowptr", "joint_sorted", "centre"):
            assert torch.equal(got[key], own[key]), (c, key)
        assert same_numbers(got["xy_sorted"].cpu().numpy(), own["xy_sorted"].cpu().numpy()), c
    size, corners, max_y = (64, 48), (5, 6, 7, 8), float(d["max_y"])
    back = back_of(ro, range(3))
    vol = ro.grain_volume(size, interp_frames=2, corner_grains=corners)
    want = volume_restated(ro, back, size, 2, range(3), "noflux", max_y, corner_grains=corners)
    assert vol.shape == (7, 48, 64) and np.array_equal(vol.cpu().numpy(), want)
    mid = ro.interp_polygons(1, 0.5)
    p = mid["xy_sorted"][:int(mid["rowptr"][1])].cpu().numpy()
    assert len(p) == 38 and ((p[:, 0] == 0) | (p[:, 0] == 1) | (p[:, 1] == 0) | (p[:, 1] == np.float32(max_y))).all()
    assert float(mid["area"][0]) < 0
