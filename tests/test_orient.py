"""Segmenting a map of full crystal orientations under cubic symmetry (ggnn_label_orientations, vectorize.label_orientations /
growth_angles / sample_from_euler_map / label_orientation_sequence / samples_from_euler_sequence) against the numpy restatement
of tests/orientcheck.py, and the restatement against the rule.

The contract.  KERNELS against RESTATEMENT: the image, n_grain, the mean quaternions and every status word equal, bit for bit.
RESTATEMENT against the RULE: the closed form of the link against the maximum over the 24 operators in float64; hand cases
at the edges of the rule; the seeded map recipe (Voronoi cells, an orientation a cell more than 5 degrees from every other,
per pixel at most 0.3 degrees of noise, a random one of the 24 equivalents and a random sign, tol = 2 degrees), where the
partition must equal the cells with every neighbour pair more than 1 degree from the threshold, so that no result hangs on a
rounding -- and where the same map falls to pieces without the symmetry and under label_grains' per-channel rule; frame 0 of
the recorded phase-field run, every grain given the orientation Rz(theta_x) Ry(theta_z) of its recorded angles.

Angles between growth directions are taken between the unit vectors (sin tz cos tx, sin tz sin tx, cos tz), the smallest over
the quarter turns about z that theta_x's % (pi/2) leaves open: theta_x alone is ill-conditioned where theta_z is small."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import labelcheck as lc
import linkcheck as lk
import orientcheck as oc
import trackcheck as tk
import vectorcheck as vc
from helpers import GOLDEN, ROOT, product_models
from graingraphnn_amd import _lib
from graingraphnn_amd import vectorize as vz
from test_label import serpentine, spiral

DEV = "cuda"
TX, TY = _lib.GGNN_LABEL_TILE_X, _lib.GGNN_LABEL_TILE_Y
BOUNDARIES = ("periodic", "noflux")
SHAPES = {(15, 65): 9, (16, 64): 9, (33, 127): 24, (3, 3): 2}       # shape -> cells: each side of a 64 x 16 tile, and the smallest
TOL = float(np.deg2rad(2.0))
DEG = np.pi / 180

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def restated(key, **kw):
    """The restatement of a named input, computed once and left unchanged."""
    return cached(("orient", key), lambda: oc.label(**kw))


def recipe(shape, boundary, seed=5):
    return cached(("recipe", shape, boundary, seed), lambda: oc.recipe(*shape, boundary, seed, n_cells=SHAPES[shape]))


def direction_angle(ax, az, bx, bz):
    """The angle between two growth directions given by their (theta_x, theta_z), up to the quarter turns about z."""
    def unit(tx, tz):
        return np.stack([np.sin(tz) * np.cos(tx), np.sin(tz) * np.sin(tx), np.cos(tz)])
    a = unit(np.asarray(ax, np.float64), np.asarray(az, np.float64))
    return np.min([np.arccos(np.clip((a * unit(np.asarray(bx, np.float64) + k * np.pi / 2, np.asarray(bz, np.float64))).sum(0), -1, 1))
                   for k in range(4)], 0)


def within_cell_pairs(cells, periodic):
    out = []
    for axis in (1, 0):
        w = cells == np.roll(cells, -1, axis)
        if not periodic:
            w[(slice(None), -1) if axis == 1 else (-1, slice(None))] = False
        out.append(w)
    return out


# ---- the rule ------------------------------------------------------------------------------------------------------------

def test_the_table_is_the_cubic_group_and_the_closed_form_its_maximum():
    ops = oc.ops64()
    assert ops.shape == (24, 4) and np.allclose((ops * ops).sum(1), 1, atol=1e-15) and np.array_equal(oc.OPS[0], [1, 0, 0, 0])
    assert set(np.unique(np.abs(oc.OPS))) == {np.float32(0), np.float32(0.5), oc.H, np.float32(1)}
    # 24 distinct rotations: no two rows equal up to sign; closed under the product up to sign
    gram = np.abs(ops @ ops.T)
    assert (gram - np.eye(24)).max() < 0.9
    for s in ops:
        prod = oc.qmul(np.broadcast_to(s[:, None], (4, 24)), np.ascontiguousarray(ops.T))
        assert np.allclose(np.sort(np.argmax(np.abs(ops @ prod), 0)), np.arange(24)) and np.abs(np.abs(ops @ prod).max(0) - 1).max() < 1e-15
    r = oc.random_quats(np.random.RandomState(1), 20000)
    m = -np.sort(-np.abs(r), axis=0)
    closed = np.maximum(m[0], np.maximum((m[0] + m[1]) * np.sqrt(0.5), 0.5 * ((m[0] + m[1]) + (m[2] + m[3]))))
    assert np.abs(closed - oc.brute_w(r)).max() <= 1e-12
    # and the float32 form on float32 inputs, against float64: a few ulp
    r32 = r.astype(np.float32)
    one = np.zeros_like(r32)
    one[0] = 1
    assert np.abs(oc.alike(one, r32, "cubic").astype(np.float64) - oc.brute_w(r32.astype(np.float64))).max() < 4e-7


def strip(*quats):
    """A 3-row map with one quaternion a column, float32 [4, 3, n]."""
    q = np.stack([np.asarray(v, np.float64) for v in quats], 1).astype(np.float32)
    return np.ascontiguousarray(np.repeat(q[:, None, :], 3, 1))


def rot(axis, degrees):
    return oc.axis_angle(np.asarray(axis, np.float64)[:, None], np.array([degrees * DEG]))[:, 0]


ONE = np.array([1.0, 0, 0, 0])


def n_components(q, tol, symmetry="cubic", **kw):
    return oc.label(q, tol, boundary="noflux", symmetry=symmetry, **kw)["status"]["n_components"]


def test_hand_cases_of_the_link():
    same = strip(ONE, rot([0, 0, 1], 90), rot([1, 1, 1], 120), ONE)       # disorientation 0 under the cubic group
    for tol in (1e-3, 0.5, 1.5):
        assert n_components(same, tol) == 1, tol
    assert n_components(same, 1.5, "none") == 4                            # 90 and 120 degrees apart without the group
    turned = strip(ONE, rot([0, 0, 1], 45), ONE)                           # 45 degrees about z: the same with and without it
    for symmetry in ("cubic", "none"):
        assert n_components(turned, 45.1 * DEG, symmetry) == 1 and n_components(turned, 44.9 * DEG, symmetry) == 3, symmetry
    # W == cos_half_tol links, the float below does not: r_w = 1 c + 0 + 0 + 0 is c itself
    tol = 0.2
    c = oc.cos_half(tol)
    for w, want in ((c, 1), (np.nextafter(c, np.float32(0)), 3)):
        edge = strip(ONE, [w, np.sqrt(1 - np.float64(w) ** 2), 0, 0], ONE)
        assert edge[0, 0, 1] == w and oc.alike(edge[:, 0, 0], edge[:, 0, 1], "cubic") == w
        assert n_components(edge, tol) == want and n_components(edge, tol, "none") == want
    assert n_components(strip(ONE, -ONE, rot([1, 2, 3], 0.5), -rot([1, 2, 3], 0.5)), 0.02) == 1      # q and -q
    bad = strip(ONE, ONE, ONE, ONE, ONE)
    bad[0, 0, 1], bad[2, 1, 2], bad[:, 2, 3] = np.nan, np.inf, np.float32(1.01) * bad[:, 2, 3]
    mask = np.ones((3, 5), np.uint8)
    mask[1, 4] = 0
    r = oc.label(bad, 0.1, valid=mask, max_sweeps=0)
    assert r["status"]["n_invalid_in"] == 4 == r["status"]["n_unfilled"] and [r["image"][y, x] for y, x in ((0, 1), (1, 2), (2, 3), (1, 4))] == [0] * 4
    assert r["status"]["n_components"] == 1 and oc.validity(strip(np.float32(1.0004) * ONE))[0, 0] and not oc.validity(strip(1.0006 * ONE))[0, 0]


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("shape", [s for s in SHAPES if s != (3, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_recipe_map_is_its_cells_with_the_symmetry_and_dust_without(shape, boundary):
    m = recipe(shape, boundary)
    periodic = boundary == "periodic"
    first = 1 if periodic else 2
    assert len(np.unique(m["cells"])) == SHAPES[shape]
    r = restated(("recipe", shape, boundary, "cubic", 1), quats=m["quats"], tol=TOL, boundary=boundary)
    margin = oc.link_margin(dict(r, quats=m["quats"], periodic=periodic), TOL)
    print(shape, boundary, "margin to the threshold in degrees:", margin / DEG)
    assert margin > 1.0 * DEG
    assert lc.same_partition(r["image"], m["cells"]) and r["n_grain"] == SHAPES[shape] + first - 1 and r["status"]["n_specks"] == 0
    within = within_cell_pairs(m["cells"], periodic)
    assert all(np.array_equal(a, b) for a, b in zip((r["right"], r["down"]), within))             # the links are exactly the cells
    # without the symmetry, and under label_grains' per-channel rule on the four components: the map falls to pieces
    n_within = sum(int(w.sum()) for w in within)
    none = restated(("recipe", shape, boundary, "none", 1), quats=m["quats"], tol=TOL, boundary=boundary, symmetry="none")
    linked = int((none["right"] & within[0]).sum() + (none["down"] & within[1]).sum())
    assert linked < 0.1 * n_within and none["n_grain"] > 20 * r["n_grain"]
    right, down = lc.links(None, m["quats"], TOL, lc.validity(angles=m["quats"]), periodic)
    per_channel = lc.label(angles=m["quats"], tol=TOL, boundary=boundary)
    assert int((right & within[0]).sum() + (down & within[1]).sum()) < 0.1 * n_within and per_channel["n_grain"] > 20 * r["n_grain"]
    # the means: within 0.3 degrees of the cell's orientation, their growth angles within 0.4 degrees of the cell's
    means = r["mean_quats"][:, first - 1:]
    cell_of = np.array([m["cells"].reshape(-1)[np.nonzero(r["image"].reshape(-1) == k + first)[0][0]] for k in range(means.shape[1])])
    truth = m["cell_quats"][:, cell_of - 1]
    assert np.abs((means.astype(np.float64) ** 2).sum(0) - 1).max() < 1e-6
    assert oc.disorientation(means, truth).max() < 0.3 * DEG
    assert direction_angle(*vz.growth_angles(means), *vz.growth_angles(truth)).max() < 0.4 * DEG
    if not periodic:
        assert r["mean_quats"][:, 0].tolist() == [1, 0, 0, 0]


def test_growth_angles():
    q = oc.random_quats(np.random.RandomState(3), 50)
    tx, tz = vz.growth_angles(q)
    assert tx.dtype == np.float64 and (tx >= 0).all() and (tx < np.pi / 2).all() and (tz >= 0).all() and tz.max() <= np.arccos(1 / np.sqrt(3)) + 1e-12
    for s in oc.ops64():
        for sign in (1.0, -1.0):
            ex, ez = vz.growth_angles(sign * oc.qmul(q, np.broadcast_to(s[:, None], q.shape)))
            assert np.abs(ez - tz).max() < 1e-12 and np.abs(np.exp(4j * ex) - np.exp(4j * tx)).max() < 4e-12
    # the direction is R(q) e_j: against the rotation of a vector by the quaternion product
    turned = []
    for j in range(3):
        e = np.zeros((4, 50))
        e[1 + j] = 1
        turned.append(oc.qmul(oc.qmul(q, e), oc.conj(q))[1:])
    turned = np.stack(turned + [-v for v in turned])                                   # [6, 3, 50]
    u = turned[np.argmax(turned[:, 2], 0), :, np.arange(50)].T
    assert np.abs(np.cos(tz) - u[2]).max() < 1e-12 and np.abs(np.exp(4j * tx) - np.exp(4j * np.arctan2(u[1], u[0]))).max() < 1e-9
    t = torch.from_numpy(q.astype(np.float32))
    a, b = vz.growth_angles(t)
    assert isinstance(a, torch.Tensor) and a.dtype == torch.float64 and np.abs(b.numpy() - tz).max() < 1e-6
    with pytest.raises(_lib.GGNNError, match="4, n"):
        vz.growth_angles(np.zeros((3, 5)))


def test_quaternions_from_bunge():
    q = vz.quaternions_from_bunge(0.0, 0.0, 0.0)
    assert q.dtype == torch.float32 and q.tolist() == [1, 0, 0, 0] and vz.growth_angles(q[:, None])[1].item() == 0
    q = vz.quaternions_from_bunge(0.0, 30.0, 0.0, degrees=True)
    assert abs(vz.growth_angles(q[:, None])[1].item() - 30 * DEG) < 1e-6
    # crystal to sample, Rz(phi1) Rx(Phi) Rz(phi2), against the product of the three turns
    rs = np.random.RandomState(4)
    a, B, c = rs.uniform(0, 2 * np.pi, (3, 5, 6)) * np.array([1, 0.5, 1])[:, None, None]
    want = oc.qmul(oc.qmul(oc.axis_angle(np.tile([[0.0], [0], [1]], 30), a.ravel()), oc.axis_angle(np.tile([[1.0], [0], [0]], 30), B.ravel())),
                   oc.axis_angle(np.tile([[0.0], [0], [1]], 30), c.ravel()))
    got = vz.quaternions_from_bunge(a, B, c)
    assert got.shape == (4, 5, 6) and np.abs(got.numpy().reshape(4, -1) - want).max() < 1e-7
    stack = vz.quaternions_from_bunge(np.stack([a, a]), np.stack([B, B]), np.stack([c, c]))
    assert stack.shape == (2, 4, 5, 6) and torch.equal(stack[1], got)
    assert np.abs(vz.quaternions_from_bunge(np.rad2deg(a), np.rad2deg(B), np.rad2deg(c), degrees=True).numpy() - got.numpy()).max() < 2e-7
    back = oc.bunge_from_quats(got.numpy().astype(np.float64))
    assert np.abs(vz.quaternions_from_bunge(*back).numpy() - got.numpy()).max() < 2e-7
    with pytest.raises(_lib.GGNNError, match="equal-shaped"):
        vz.quaternions_from_bunge(a, B[:2], c)


# ---- the recorded frame ----------------------------------------------------------------------------------------------------

def golden():
    def make():
        d = np.load(os.path.join(GOLDEN, "pf_frames_cfg1.npz"))
        frame = d["frames"][0].astype(np.int32)
        tx, tz = d["theta_x"].astype(np.float64), d["theta_z"].astype(np.float64)
        n = len(tx)
        grain_quats = oc.qmul(oc.axis_angle(np.tile([[0.0], [0], [1]], n), tx), oc.axis_angle(np.tile([[0.0], [1], [0]], n), tz))
        rs = np.random.RandomState(7)
        quats = oc.in_variants(grain_quats[:, frame.reshape(-1) - 1], rs).reshape(4, *frame.shape)
        return {"frame": frame, "clean": lc.relabel_by_first_pixel(frame), "theta": np.stack([tx, tz]), "grain_quats": grain_quats,
                "quats": np.ascontiguousarray(quats), "G": float(d["G"]), "R": float(d["R"])}
    return cached("golden", make)


GOLDEN_TOL = 1e-3


def test_the_recorded_frame_as_orientations_in_random_equivalents():
    g = golden()
    frame = g["frame"]
    # no two neighbouring grains within 2 tol of each other (one seed of equivalents, one frame: nothing is dropped)
    pairs = np.unique(np.concatenate([np.stack([frame, np.roll(frame, -1, a)]).reshape(2, -1) for a in (0, 1)], 1), axis=1)
    pairs = pairs[:, pairs[0] != pairs[1]]
    apart = oc.disorientation(g["grain_quats"][:, pairs[0] - 1], g["grain_quats"][:, pairs[1] - 1])
    print("neighbouring grains:", pairs.shape[1], "the closest pair in rad:", apart.min())
    assert apart.min() > 2 * GOLDEN_TOL
    r = restated("golden", quats=g["quats"], tol=GOLDEN_TOL)
    print(r["status"])
    assert np.array_equal(r["image"], g["clean"]) and r["n_grain"] == 118 and r["status"]["n_components"] == 118
    v = vc.vectorize(r["image"], 118, "points")
    assert vc.is_valid(v["status"]) and v["status"]["n_joint"] == 236
    first = np.array([np.nonzero(g["clean"].reshape(-1) == k + 1)[0][0] for k in range(118)])
    want = g["theta"][:, frame.reshape(-1)[first] - 1]
    tx, tz = vz.growth_angles(r["mean_quats"])
    keep = want[1] < 44 * DEG
    err_x = np.abs(np.exp(4j * tx[keep]) - np.exp(4j * want[0][keep])) / 4
    print("grains kept:", int(keep.sum()), "worst theta_x:", err_x.max(), "worst theta_z:", np.abs(tz - want[1])[keep].max(),
          "smallest theta_z:", want[1][keep].min())
    assert keep.sum() == 55 and np.abs(tz - want[1])[keep].max() < 1e-5 and err_x.max() < 1e-5


# ---- the entry point on the host ---------------------------------------------------------------------------------------------

def test_entry_point_validates_on_the_host():
    lib = _lib.load()
    assert lib.ggnn_version() == 26 == _lib.GGNN_ABI_VERSION
    assert {"ggnn_label_orientations", "ggnn_label_orient_workspace_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    assert lib.ggnn_label_orientations(None, None) == -1
    assert lib.ggnn_label_orient_workspace_bytes(2, 8) == 0 and lib.ggnn_label_orient_workspace_bytes(8, 1 << 15) == 0
    need = lib.ggnn_label_orient_workspace_bytes(32, 32)
    assert need == lib.ggnn_label_workspace_bytes(32, 32, 4) >= 32 * 32 * (21 + 32)
    buf = (ctypes.c_int64 * 64)()                 # (host memory: refused before anything would be launched)
    p = ctypes.cast(buf, ctypes.c_void_p)
    c = float(oc.cos_half(0.03))

    def call(**kw):
        A = _lib.LabelOrientArgs(p, None, p, p, p, p, need, 32, 32, 64, 1, c, _lib.GGNN_SYM_CUBIC, 4, 0)
        A.image = None                            # (so that a call that passes every other check still launches nothing)
        for k, v in kw.items():
            setattr(A, k, v)
        return lib.ggnn_label_orientations(ctypes.byref(A), None)
    assert call() == -1
    for bad in (dict(quats=None), dict(mean_quats=None), dict(status=None), dict(workspace=None), dict(nx=2), dict(ny=2), dict(nx=1 << 15),
                dict(ny=1 << 15), dict(cos_half_tol=float(oc.cos_half(np.pi / 2))), dict(cos_half_tol=0.5), dict(cos_half_tol=1.0000001),
                dict(cos_half_tol=float("nan")), dict(cos_half_tol=-0.9), dict(symmetry=2), dict(symmetry=-1), dict(boundary=2),
                dict(min_pixels=0), dict(max_sweeps=-1), dict(max_sweeps=_lib.GGNN_LABEL_MAX_SWEEPS + 1), dict(grain_capacity=0),
                dict(grain_capacity=2 ** 31 - 1), dict(status=p.value + 4), dict(workspace=p.value + 4), dict(mean_quats=p.value + 2),
                dict(quats=p.value + 2), dict(workspace_bytes=need - 1)):
        assert call(image=p, **bad) == -1, bad
    assert call(image=p.value + 2) == -1


def test_header_binding_and_restatement_agree():
    src = open(os.path.join(ROOT, "include", "ggnn.h")).read()
    for name in ("GGNN_SYM_NONE", "GGNN_SYM_CUBIC", "GGNN_ORIENT_OPS"):
        assert f"#define {name} {getattr(_lib, name)}\n" in src, name
    assert "#define GGNN_ORIENT_H 0.70710678f\n" in src and np.float32(_lib.GGNN_ORIENT_H) == oc.H
    body = re.search(r"typedef struct ggnn_label_orient_args \{(.*?)\} ggnn_label_orient_args;", src, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in _lib.LabelOrientArgs._fields_]
    assert ctypes.sizeof(_lib.LabelOrientArgs) == 7 * 8 + 4 * 8 + 4 * 4
    assert vz.SYMMETRIES == {"none": _lib.GGNN_SYM_NONE, "cubic": _lib.GGNN_SYM_CUBIC}
    # the operator table the header lists is the restatement's, entry for entry
    rows = re.findall(r"s_(\d+) = \(([^)]*)\)", src)
    assert [int(i) for i, _ in rows] == list(range(24))
    value = {"0": 0.0, "1": 1.0, "h": float(oc.H), "-h": -float(oc.H), "0.5": 0.5, "-0.5": -0.5}
    table = np.array([[value[t.strip()] for t in row.split(",")] for _, row in rows], np.float32)
    assert np.array_equal(table, oc.OPS)
    kernel = open(os.path.join(ROOT, "graingraphnn_amd", "csrc", "label.hip")).read()
    body = re.search(r"ORIENT_OPS\[GGNN_ORIENT_OPS\]\[4\] = \{(.*?)\};", kernel, re.S).group(1)
    tokens = re.findall(r"-?GGNN_ORIENT_H|-?\d+(?:\.\d+)?f?", body)
    device = np.array([(-1 if t.startswith("-") else 1) * float(oc.H) if "ORIENT_H" in t else float(t.rstrip("f")) for t in tokens], np.float32)
    assert np.array_equal(device.reshape(24, 4), oc.OPS)


def test_python_entry_points_refuse_what_they_cannot_take():
    host = torch.zeros(4, 8, 8)
    for args, kw, match in (((host, 0.03), {}, "device"), ((host, 0.03), dict(boundary="open"), "boundary"),
                            ((host, 0.03), dict(symmetry="hexagonal"), "symmetry"), ((host, 0.0), {}, "tol"), ((host, np.pi / 2), {}, "tol"),
                            ((host, float(np.nextafter(np.pi / 2, 0))), {}, "rounds to")):
        with pytest.raises(_lib.GGNNError, match=match):
            vz.label_orientations(*args, **kw)
    with pytest.raises(_lib.GGNNError, match="match_tol"):
        vz.label_orientation_sequence(host[None], 0.03, match_tol=0.1)
    with pytest.raises(_lib.GGNNError, match="device"):
        vz.label_orientation_sequence(host[None], 0.03)


# ---- GPU: the kernels equal the restatement bit for bit ----------------------------------------------------------------------

def to_dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(kw):
    """label_orientations on the device for the restatement's keywords."""
    return vz.label_orientations(**{k: (to_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()})


def assert_equals_restatement(got, r, what):
    image, n_grain, means, status = got
    print(what, status)
    assert status == r["status"], (what, status, r["status"])
    assert status["n_bound_hits"] == 0 and n_grain == r["n_grain"], what
    assert image.dtype == torch.int32 and np.array_equal(image.cpu().numpy(), r["image"]), what
    assert means.dtype == torch.float32 and means.shape == r["mean_quats"].shape, what
    assert np.array_equal(means.cpu().numpy().view(np.uint32), r["mean_quats"].view(np.uint32)), what


def noisy_recipe(shape, boundary, seed=5):
    """The recipe with 1 % of the pixels re-drawn at random (specks) and 1 % not indexed (NaN)."""
    def make():
        q = recipe(shape, boundary, seed)["quats"].copy()
        rs = np.random.RandomState(seed + 100)
        u = rs.rand(*shape)
        if shape == (3, 3):
            u[1, 1], u[0, 2] = 0.005, 0.015                # (1 % of nine pixels: one each, so that the sweeps run here too)
        speck = u < 0.01
        q[:, speck] = oc.random_quats(rs, int(speck.sum())).astype(np.float32)
        q[:, (u >= 0.01) & (u < 0.02)] = np.nan
        return q
    return cached(("noisy", shape, boundary, seed), make)


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("shape", sorted(SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_recipe_maps_on_the_device(shape, boundary):
    for name, q in (("clean", recipe(shape, boundary)["quats"]), ("noisy", noisy_recipe(shape, boundary))):
        for symmetry in ("cubic", "none"):
            for mp in (1, 3):
                kw = dict(quats=q, tol=TOL, min_pixels=mp, boundary=boundary, symmetry=symmetry)
                r = restated((name, shape, boundary, symmetry, mp), **kw)
                if name == "noisy" and symmetry == "cubic" and mp == 3 and shape != (3, 3):
                    assert r["status"]["n_specks"] > 0 and r["status"]["n_invalid_in"] > 0 and r["status"]["n_sweeps"] >= 1
                assert_equals_restatement(run(kw), r, (name, shape, boundary, symmetry, mp))


PATHS = {"serpentine": lambda: serpentine(2 * TY + 1, 3 * TX + 1), "spiral": lambda: spiral(2 * TY + 1, 3 * TX + 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PATHS))
def test_one_component_half_the_image_long(name):
    path = PATHS[name]()
    ny, nx = path.shape
    q = oc.recipe(ny, nx, "periodic", 8, seeds=[(0.0, 0.0)])["quats"]        # one orientation, noise, random equivalents
    q[:, path == 0] = np.nan
    for boundary in BOUNDARIES:
        kw = dict(quats=q, tol=TOL, boundary=boundary, max_sweeps=0)
        r = restated(("path", name, boundary), **kw)
        want = 2 if name == "spiral" and boundary == "noflux" else 1                  # (the spiral closes through the wrap alone)
        assert r["status"]["n_components"] == want and r["status"]["n_unfilled"] == int((path == 0).sum()), (name, boundary)
        assert_equals_restatement(run(kw), r, (name, boundary))


@pytest.mark.gpu
@pytest.mark.parametrize("boundary,shape", [("periodic", (TY, TX)), ("noflux", (TY - 1, TX + 1))])
def test_every_pixel_its_own_grain(boundary, shape):
    ny, nx = shape
    two = np.stack([ONE, rot([1, 2, 3], 30)], 1).astype(np.float32)
    q = np.ascontiguousarray(two[:, (np.add.outer(np.arange(ny), np.arange(nx)) % 2)])
    for cap in (None, ny * nx // 2 + 3):
        kw = dict(quats=q, tol=TOL, boundary=boundary, grain_capacity=cap)
        r = restated(("checkerboard", shape, boundary, cap), **kw)
        assert r["status"]["n_grains"] == ny * nx and r["status"]["overflow"] == int(cap is not None)
        assert np.array_equal(r["image"].reshape(-1), np.arange(ny * nx) + (1 if boundary == "periodic" else 2))
        got = run(kw)
        assert_equals_restatement(got, r, (boundary, shape, cap))
        if cap is not None:
            assert got[2].shape == (4, cap)


GUARD = 64


def guarded_call(quats, mask, tol, min_pixels, max_sweeps, boundary, cap, symmetry="cubic"):
    """The entry point itself with GUARD canary words or 256 bytes before and after the image, the means, the status and the
    workspace -> (image, means, status) with their guards, and whether the workspace's guards survived."""
    lib = _lib.load()
    ny, nx = quats.shape[1:]
    need = lib.ggnn_label_orient_workspace_bytes(nx, ny)
    image = torch.full((ny * nx + 2 * GUARD,), -7, dtype=torch.int32, device=DEV)
    means = torch.full((4 * cap + 2 * GUARD,), -7.0, dtype=torch.float32, device=DEV)
    status = torch.full((9 + 2 * GUARD,), -7, dtype=torch.int64, device=DEV)
    ws = torch.full((need + 2 * 256,), 0x5A, dtype=torch.uint8, device=DEV)
    d_q, d_mask = to_dev(quats), None if mask is None else to_dev(mask.astype(np.uint8))
    A = _lib.LabelOrientArgs(_lib.ptr(d_q), _lib.ptr(d_mask), image[GUARD:].data_ptr(), means[GUARD:].data_ptr(), status[GUARD:].data_ptr(),
                             ws[256:].data_ptr(), need, nx, ny, cap, min_pixels, float(oc.cos_half(tol)), vz.SYMMETRIES[symmetry], max_sweeps,
                             vz.BOUNDARIES[boundary])
    _lib.check(lib.ggnn_label_orientations(ctypes.byref(A), _lib.current_stream()), "ggnn_label_orientations")
    torch.cuda.synchronize()
    return image, means, status, bool((ws[:256] == 0x5A).all()) and bool((ws[256 + need:] == 0x5A).all())


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_guarded_arrays_and_a_capacity_inside_the_grains(boundary):
    shape = (33, 127)
    ny, nx = shape
    q = noisy_recipe(shape, boundary)
    mask = np.ones(shape, np.uint8)
    mask[3:6, 60:70] = 0
    full = oc.label(q, TOL, valid=mask, min_pixels=3, boundary=boundary)
    for cap in (full["n_grain"] - 2, full["n_grain"] + 5):
        r = oc.label(q, TOL, valid=mask, min_pixels=3, boundary=boundary, grain_capacity=cap)
        image, means, status, ws_ok = guarded_call(q, mask, TOL, 3, 64, boundary, cap)
        assert ws_ok and dict(zip(lc.STATUS, status[GUARD:GUARD + 9].tolist())) == r["status"], cap
        assert r["status"]["overflow"] == int(cap < full["n_grain"])
        assert bool((status[:GUARD] == -7).all()) and bool((status[GUARD + 9:] == -7).all())
        assert bool((image[:GUARD] == -7).all()) and bool((image[GUARD + ny * nx:] == -7).all())
        assert np.array_equal(image[GUARD:GUARD + ny * nx].cpu().numpy(), r["image"].reshape(-1))
        n = min(cap, r["n_grain"])
        rows = means[GUARD:GUARD + 4 * cap].view(4, cap)
        assert np.array_equal(rows[:, :n].cpu().numpy().view(np.uint32), r["mean_quats"].view(np.uint32))
        assert bool((rows[:, n:] == -7).all()) and bool((means[:GUARD] == -7).all()) and bool((means[GUARD + 4 * cap:] == -7).all())


@pytest.mark.gpu
def test_two_runs_and_a_captured_graph_give_the_same_bits():
    shape = (33, 127)
    q = noisy_recipe(shape, "periodic")
    r = restated(("noisy", shape, "periodic", "cubic", 3), quats=q, tol=TOL, min_pixels=3, boundary="periodic", symmetry="cubic")
    args = (to_dev(q), TOL, None, 3, 64, "periodic", None, "cubic")
    first, second = vz._label_orient(*args), vz._label_orient(*args)      # (also the warm-up of the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = vz._label_orient(*args)
    graph.replay()                                                        # (a replay starts from its own zeroed words and sums)
    torch.cuda.synchronize()
    once = {k: held[k].clone() for k in ("image", "means", "status")}
    graph.replay()
    torch.cuda.synchronize()
    for k in ("image", "means", "status"):
        assert torch.equal(first[k], second[k]) and torch.equal(first[k], once[k]) and torch.equal(first[k], held[k]), k
    assert dict(zip(lc.STATUS, held["status"].tolist())) == r["status"] and np.array_equal(held["image"].cpu().numpy(), r["image"])
    n = r["n_grain"]
    assert np.array_equal(held["means"][:, :n].cpu().numpy().view(np.uint32), r["mean_quats"].view(np.uint32))


def assert_same_sample(a, b):
    for da, db in zip(a, b):
        assert da.keys() == db.keys()
        for k in da:
            assert da[k].dtype == db[k].dtype and torch.equal(da[k], db[k]), k


class Counted:
    """Counts the calls that bring a device tensor to the host."""
    NAMES = ("tolist", "cpu", "item", "numpy")

    def __init__(self, monkeypatch):
        self.n = 0
        for name in self.NAMES:
            monkeypatch.setattr(torch.Tensor, name, self.wrap(getattr(torch.Tensor, name)))

    def wrap(self, f):
        def counted(t, *a, **kw):
            self.n += bool(t.is_cuda)
            return f(t, *a, **kw)
        return counted


def euler_maps(quats):
    """Euler angles (float64, on the device) whose quaternions are `quats` up to the rounding of the round trip, and the
    float32 quaternions the package forms from them, back on the host: what the restatement is given."""
    angles = [to_dev(a) for a in oc.bunge_from_quats(np.asarray(quats, np.float64))]
    return angles, vz.quaternions_from_bunge(*angles).cpu().numpy()


@pytest.mark.gpu
@torch.no_grad()
def test_sample_from_euler_map_periodic_and_ten_rollout_steps(monkeypatch):
    from graingraphnn_amd import GrainRollout
    g = golden()
    angles, q = euler_maps(g["quats"])
    r = oc.label(q, GOLDEN_TOL)
    assert np.array_equal(r["image"], g["clean"])
    with monkeypatch.context() as m:
        counted = Counted(m)
        image, n_grain, means, status = vz.label_orientations(to_dev(q), GOLDEN_TOL)
        assert counted.n == 1                                             # one read-back
    assert_equals_restatement((image, n_grain, means, status), r, "golden")
    kw = dict(span=6, patch_pixels=501 ** 2, grid="points")
    X, EI, EA, image, status = vz.sample_from_euler_map(*angles, g["G"], g["R"], GOLDEN_TOL, **kw)
    assert np.array_equal(image.cpu().numpy(), r["image"]) and {k: status[k] for k in lc.STATUS} == r["status"]
    assert np.array_equal(status["mean_quats"].cpu().numpy().view(np.uint32), r["mean_quats"].view(np.uint32))
    tx, tz = (a.astype(np.float32) for a in vz.growth_angles(r["mean_quats"]))
    assert np.array_equal(status["theta_x"], tx) and np.array_equal(status["theta_z"], tz) and status["theta_x"].dtype == np.float32
    assert_same_sample((X, EI, EA), vz.sample_from_image(image, tx, tz, g["G"], g["R"], **kw))
    assert X["grain"].shape == (118, 11) and X["joint"].shape == (236, 8)
    R, Cm = product_models(10020, 1.0, DEV)
    ro = GrainRollout(R, Cm, X, EI, EA, 6, refresh_centres=True)
    for _ in range(10):
        pred = ro.step()
        assert all(bool(torch.isfinite(t).all()) for t in pred.values())
    assert not ro.range_exceeded()


@pytest.mark.gpu
@torch.no_grad()
def test_sample_from_euler_map_on_the_noflux_golden():
    field = np.load(os.path.join(GOLDEN, "grain_image_cfg1.npz"))["noflux__alpha_field"].astype(np.int32)
    rs = np.random.RandomState(7)
    grain_quats = oc.random_quats(rs, 102)
    pairs = np.unique(np.concatenate([np.stack([field[:-1], field[1:]]).reshape(2, -1), np.stack([field[:, :-1], field[:, 1:]]).reshape(2, -1)], 1), axis=1)
    pairs = pairs[:, pairs[0] != pairs[1]]
    assert oc.disorientation(grain_quats[:, pairs[0]], grain_quats[:, pairs[1]]).min() > 2 * TOL
    angles, q = euler_maps(oc.in_variants(grain_quats[:, field.reshape(-1)], rs).reshape(4, *field.shape))
    r = oc.label(q, TOL, boundary="noflux")
    assert r["n_grain"] == 101 and np.array_equal(r["image"], lc.relabel_by_first_pixel(field) + 1)
    kw = dict(span=6, patch_pixels=501 ** 2, grid="points", boundary="noflux")
    X, EI, EA, image, status = vz.sample_from_euler_map(*angles, 2.0, 0.5, TOL, **kw)
    assert np.array_equal(image.cpu().numpy(), r["image"]) and {k: status[k] for k in lc.STATUS} == r["status"]
    assert np.array_equal(status["mean_quats"].cpu().numpy().view(np.uint32), r["mean_quats"].view(np.uint32))
    assert status["mean_quats"][:, 0].tolist() == [1, 0, 0, 0] and status["theta_z"][0] == 0
    tx, tz = (a.astype(np.float32) for a in vz.growth_angles(r["mean_quats"]))
    assert np.array_equal(status["theta_x"], tx) and np.array_equal(status["theta_z"], tz)
    assert_same_sample((X, EI, EA), vz.sample_from_image(image, tx, tz, 2.0, 0.5, **kw))
    assert X["grain"].shape == (101, 11) and X["joint"].shape == (198, 8)


def drifting_frames(shape, boundary, T=3, seed=9):
    """T frames of the recipe: the seeds drift by up to a pixel a frame, the cells keep their orientations, every frame draws
    its own noise and its own random equivalents."""
    def make():
        ny, nx = shape
        seeds = tk.moving_seeds(ny, nx, 4, T, seed, drift=1.0)
        first = oc.recipe(ny, nx, boundary, seed, seeds=seeds[0])
        frames = [first] + [oc.recipe(ny, nx, boundary, seed + t, seeds=seeds[t], cell_quats=first["cell_quats"]) for t in range(1, T)]
        return {"cells": np.stack([f["cells"] for f in frames]), "quats": np.stack([f["quats"] for f in frames])}
    return cached(("drifting", shape, boundary, T, seed), make)


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_a_sequence_keeps_its_ids_through_fresh_equivalents(boundary, monkeypatch):
    shape, T = (33, 127), 3
    d = drifting_frames(shape, boundary, T)
    noflux = boundary == "noflux"
    cap = 300
    per_frame = [oc.label(d["quats"][t], TOL, boundary=boundary, grain_capacity=cap) for t in range(T)]
    labels = np.stack([r["image"] for r in per_frame])
    means = np.zeros((T, 4, cap), np.float32)
    for t, r in enumerate(per_frame):
        means[t, :, :r["mean_quats"].shape[1]] = r["mean_quats"]
    Lc = cap - 1 if noflux else cap
    want = lk.link(labels, [r["status"]["n_grains"] for r in per_frame], means=np.ascontiguousarray(means[:, :, 1:] if noflux else means),
                   boundary=boundary, local_capacity=Lc)
    assert lc.same_partition(want["frames"], d["cells"]) and want["n_global"] == 16        # one id a cell through the three frames
    assert not np.array_equal(labels[0], labels[T - 1])
    quats = to_dev(d["quats"])
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        counted = Counted(m)
        frames, n_grain, quat, report = vz.label_orientation_sequence(quats, TOL, boundary=boundary, grain_capacity=cap)
        assert counted.n == 1                                             # one read-back
    assert n_grain == want["n_grain"] == 16 + noflux and report["label"] == [r["status"] for r in per_frame] and report["frames"] == want["status"]
    assert np.array_equal(frames.cpu().numpy(), want["frames"])
    theta = want["theta"][:, :16]
    assert np.array_equal(quat.cpu().numpy().view(np.uint32), per_frame[0]["mean_quats"].view(np.uint32))   # the first frame's means
    assert np.array_equal(quat[:, int(noflux):].cpu().numpy().view(np.uint32), theta.view(np.uint32))
    # the training set in one call, from the Euler angles
    angles = [to_dev(a) for a in oc.bunge_from_quats(d["quats"].astype(np.float64).transpose(1, 0, 2, 3))]
    kw = dict(patch_pixels=shape[0] * shape[1], grid="points", boundary=boundary)
    samples, rep, out = vz.samples_from_euler_sequence(*angles, 2.0, 0.4, TOL, grain_capacity=cap, **kw)
    seq = rep["sequence"]
    assert lc.same_partition(out.cpu().numpy(), d["cells"]) and seq["quat"].shape == (4, 16 + noflux)
    tx, tz = (a.cpu().numpy().astype(np.float32) for a in vz.growth_angles(seq["quat"]))
    assert np.array_equal(seq["theta_x"], tx) and np.array_equal(seq["theta_z"], tz)
    again, again_rep = vz.frames_to_samples(out, tx, tz, 2.0, 0.4, **kw)
    assert rep["pairs"] == again_rep["pairs"] and rep["counts"] == again_rep["counts"] and len(samples) == len(again)
    for a, b in zip(samples, again):
        assert_same_sample(a, b)
