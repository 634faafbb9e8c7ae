"""Segmenting an orientation map into a grain-ID image (ggnn_label_grains, vectorize.label_grains / sample_from_orientations)
against the numpy restatement of tests/labelcheck.py, and the restatement against hand-drawn images, scipy.ndimage.label and
the recorded phase-field frames.

The contract.  KERNELS against RESTATEMENT: the image, n_grain, the mean angles and every status word equal, bit for bit, with
n_bound_hits 0 everywhere.  RESTATEMENT against the RULE: one hand-drawn image per clause of include/ggnn.h's rule; against
scipy's labelling as partitions; on frame 0 of pf_frames_cfg1.npz with the issue's noise recipe it reproduces the recorded
table (grains, sweeps, unfilled, the vectoriser's status, pixels that differ from the clean relabelled frame).

The no-flux end-to-end case.  grain_image_cfg1.npz's `noflux__alpha_pde` holds only zeros (the reference records no
phase-field image for its no-flux run), so there is nothing in it to segment: the test pins that (every pixel unfilled,
sample_from_orientations raises) and runs the end-to-end comparison on the same record's `noflux__alpha_field`, the no-flux
structure itself (ids 2 .. 101, 198 junctions)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import labelcheck as lc
import trackcheck as tk
import vectorcheck as vc
import vectorcheck_noflux as vn
from helpers import GOLDEN, ROOT, product_models
from graingraphnn_amd import _lib
from graingraphnn_amd import vectorize as vz
from graingraphnn_amd.synthetic import EDGE_TYPES

DEV = "cuda"
TX, TY = _lib.GGNN_LABEL_TILE_X, _lib.GGNN_LABEL_TILE_Y
BOUNDARIES = ("periodic", "noflux")
NOISE = {(0.01, 0): (118, 1, 0, 29), (0.04, 1): (118, 1, 0, 131), (0.10, 2): (118, 2, 0, 423)}   # grains, sweeps, unfilled, differing

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def restated(key, **kw):
    """The restatement of a named input, computed once and left unchanged."""
    return cached(("label", key), lambda: lc.label(**kw))


def f32(a):
    return np.asarray(a, np.float32)


# ---- the golden frames ---------------------------------------------------------------------------------------------------

def golden():
    def make():
        d = np.load(os.path.join(GOLDEN, "pf_frames_cfg1.npz"))
        frames = d["frames"].astype(np.int32)
        theta = np.stack([d["theta_x"], d["theta_z"]]).astype(np.float32)
        return {"frames": frames, "theta": theta, "clean": lc.relabel_by_first_pixel(frames[0]), "G": float(d["G"]), "R": float(d["R"])}
    return cached("golden", make)


def golden_inputs(tag):
    """tag "clean" or a (d, seed) of NOISE -> (ids, angles, min_pixels)."""
    g = golden()
    if tag == "clean":
        return g["frames"][0], g["theta"][:, g["frames"][0] - 1], 1
    ids, angles = cached(("noisy", tag), lambda: lc.noisy(g["frames"][0], g["theta"], *tag))
    return ids, angles, 8


def golden_restated(tag, mode):
    ids, angles, mp = golden_inputs(tag)
    kw = dict(ids=ids) if mode == "ids" else dict(angles=angles, tol=1e-3)
    return restated(("golden", tag, mode), min_pixels=mp, **kw), dict(kw, min_pixels=mp)


# ---- hand-drawn cases: one per clause of the rule -> (keywords of label, check(result)) ------------------------------------

TOL = np.float32(0.25)


def rows(*r):
    return np.array(r, np.int32)


def hand_cases():
    c = {}
    col = lambda v: f32(np.tile(v, (3, 1)))[None]

    def links_at_tol(r):
        assert r["status"]["n_components"] == 1 and r["n_grain"] == 2 and (r["image"] == 2).all()
    c["a difference of tol links"] = (dict(angles=col([0.0, TOL, 0.0]), tol=TOL, boundary="noflux"), links_at_tol)

    def not_beyond(r):
        assert r["status"]["n_components"] == 3 and r["image"].tolist() == [[2, 3, 4]] * 3
    c["nextafter(tol) does not link"] = (dict(angles=col([0.0, np.nextafter(TOL, np.float32(1)), 0.0]), tol=TOL, boundary="noflux"), not_beyond)

    def ramp(r):
        assert r["status"]["n_components"] == 1 and r["status"]["n_grains"] == 1 and (r["image"] == 2).all()
        assert r["mean_angles"][0, 1] == np.float32(11 * 0.25 / 2)
    c["a ramp is one component"] = (dict(angles=col(np.arange(12) * TOL), tol=TOL, boundary="noflux"), ramp)

    bad = np.ones((1, 3, 5), np.float32)
    bad[0, 0, 1], bad[0, 1, 3], bad[0, 2, 0], bad[0, 2, 4], bad[0, 1, 1] = np.nan, np.inf, -np.inf, 8.5, 8.0

    def invalid(r):
        s = r["status"]
        assert s["n_invalid_in"] == 4 == s["n_unfilled"] and s["n_components"] == 2 and s["n_sweeps"] == 0
        assert [r["image"][y, x] for y, x in ((0, 1), (1, 3), (2, 0), (2, 4))] == [0] * 4 and r["image"][1, 1] == 2 and r["image"][0, 0] == 1
    c["nan, inf and beyond 8 are invalid"] = (dict(angles=bad, tol=TOL, max_sweeps=0), invalid)

    def masked(r):
        assert r["status"]["n_invalid_in"] == 3 and (r["image"][:, 1] == 0).all() and r["status"]["n_components"] == 2
    c["the mask makes a pixel invalid"] = (dict(ids=np.ones((3, 3), np.int32), valid=rows([1, 0, 1], [1, 0, 1], [1, 0, 1]), boundary="noflux",
                                               max_sweeps=0), masked)

    def smaller_root(r):
        assert r["image"].tolist() == [[2, 2, 2, 3, 3]] * 3 and r["status"]["n_sweeps"] == 1
    c["one neighbour each: the smaller root"] = (dict(ids=np.tile(rows([5, 5, 0, 4, 4]), (3, 1)), boundary="noflux"), smaller_root)

    def majority(r):   # (1, 1): left root 0, right and up root 1, down open; (2, 1): left root 0, right root 1: the smaller
        assert r["image"].tolist() == [[2, 3, 3, 3], [2, 3, 3, 3], [2, 2, 3, 3]] and r["status"]["n_sweeps"] == 1
        assert r["state"][1, 1] == 1 and r["state"][2, 1] == 0
    c["two against one: the majority"] = (dict(ids=rows([2, 1, 1, 1], [2, 0, 1, 1], [2, 0, 1, 1]), boundary="noflux"), majority)

    block = np.ones((7, 7), np.int32)
    block[2:5, 2:5] = 0

    def two_sweeps(r):
        assert r["status"]["n_sweeps"] == 2 and r["status"]["n_unfilled"] == 0 and (r["image"] == 1).all() and r["status"]["n_invalid_in"] == 9
    c["a 3 x 3 invalid block needs two sweeps"] = (dict(ids=block), two_sweeps)

    def one_sweep(r):
        assert r["status"]["n_sweeps"] == 1 and r["status"]["n_unfilled"] == 1 and r["image"][3, 3] == 0 and int((r["image"] == 1).sum()) == 48
    c["max_sweeps 1 leaves its centre"] = (dict(ids=block, max_sweeps=1), one_sweep)

    def jacobi(r):     # Gauss-Seidel in raster order would give 2 2 2 2 3 3
        assert r["image"].tolist() == [[2, 2, 2, 3, 3, 3]] * 3 and r["status"]["n_sweeps"] == 2
    c["a strip of four between two grains: jacobi"] = (dict(ids=np.tile(rows([1, 0, 0, 0, 0, 2]), (3, 1)), boundary="noflux"), jacobi)

    def nothing(r):
        s = r["status"]
        assert s["n_unfilled"] == 12 and s["n_sweeps"] == 0 and r["n_grain"] == 0 and not r["image"].any() and s["n_grains"] == 0
    c["no closed neighbour: unfilled"] = (dict(ids=np.zeros((3, 4), np.int32)), nothing)

    def specks_only(r):
        s = r["status"]
        assert s["n_specks"] == 2 and s["n_speck_pixels"] == 9 and s["n_unfilled"] == 9 and r["n_grain"] == 1 and s["n_components"] == 2
    c["specks alone stay unfilled"] = (dict(ids=rows([1, 1, 2], [1, 1, 2], [1, 2, 2]), min_pixels=6, boundary="noflux"), specks_only)

    numbered = rows([7, 7, 3], [7, 3, 3], [5, 5, 5])

    def walls_numbering(r):
        assert r["image"].tolist() == [[2, 2, 3], [2, 3, 3], [4, 4, 4]] and r["n_grain"] == 4 and r["status"]["n_grains"] == 3
    c["numbering by root, walls from 2"] = (dict(ids=numbered, boundary="noflux"), walls_numbering)

    def periodic_numbering(r):   # rows 0 and 2 are neighbours through the wrap, but 7 != 5
        assert r["image"].tolist() == [[1, 1, 2], [1, 2, 2], [3, 3, 3]] and r["n_grain"] == 3
    c["numbering by root, periodic from 1"] = (dict(ids=numbered), periodic_numbering)

    a = np.zeros((2, 4, 6), np.float32)
    a[0, :, :3], a[0, :, 3:], a[1, :, :3], a[1, :, 3:] = 0.3125, 1.125, 0.75, 0.1875   # (exact in the fixed point)
    a[:, 1, 1] = (1.5, 1.375)      # a speck inside the left grain
    a[:, 2, 4] = np.nan            # a non-indexed point inside the right one

    def means(r):
        assert r["image"].tolist() == [[2, 2, 2, 3, 3, 3]] * 4 and r["status"]["n_specks"] == 1 and r["status"]["n_invalid_in"] == 1
        assert r["mean_angles"].tolist() == [[0.0, 0.3125, 1.125], [0.0, 0.75, 0.1875]]
    c["absorbed pixels do not move the means"] = (dict(angles=a, tol=1e-3, min_pixels=2, boundary="noflux"), means)
    return c


def wrap_cases():
    """name -> (ids, components when periodic, components with walls)."""
    x = np.tile(rows([1, 2, 2, 3, 3, 1]), (5, 1))
    corner = np.full((6, 6), 2, np.int32)
    corner[0, 0] = corner[0, 5] = corner[5, 0] = corner[5, 5] = 1
    return {"through the x wrap": (x, 3, 4), "through the y wrap": (np.ascontiguousarray(x.T), 3, 4), "through both: a corner": (corner, 2, 5)}


HAND = hand_cases()
WRAP = wrap_cases()


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_drawn_clauses_of_the_rule(name):
    kw, check = HAND[name]
    r = restated(("hand", name), **kw)
    check(r)
    assert r["status"]["n_bound_hits"] == 0 and r["image"].dtype == np.int32


@pytest.mark.parametrize("name", sorted(WRAP))
def test_wrap_cases(name):
    ids, n_periodic, n_walls = WRAP[name]
    p, w = restated(("wrap", name, "periodic"), ids=ids), restated(("wrap", name, "noflux"), ids=ids, boundary="noflux")
    assert p["status"]["n_components"] == n_periodic == p["n_grain"] and w["status"]["n_components"] == n_walls == w["n_grain"] - 1
    assert p["image"][0, 0] == p["image"][-1, -1] == 1 and w["image"][0, 0] == 2 and w["image"][-1, -1] == n_walls + 1


def scipy_partition(ids, periodic):
    """scipy.ndimage.label per id, the labels of the two wraps merged by hand when periodic."""
    from scipy import ndimage
    out, n = np.zeros(ids.shape, np.int64), 0
    for v in np.unique(ids[ids > 0]):
        lab, k = ndimage.label(ids == v)
        out[lab > 0] = lab[lab > 0] + n
        n += k
    if periodic:
        parent = list(range(n + 1))

        def find(a):
            while parent[a] != a:
                a = parent[a]
            return a
        for a, b, ia, ib in ((out[:, 0], out[:, -1], ids[:, 0], ids[:, -1]), (out[0], out[-1], ids[0], ids[-1])):
            for la, lb, va, vb in zip(a, b, ia, ib):
                if va == vb and va > 0:
                    ra, rb = find(int(la)), find(int(lb))
                    parent[max(ra, rb)] = min(ra, rb)
        out = np.array([find(a) for a in range(n + 1)])[out]
    return out


def blobs(ny, nx, n_ids, seed, holes=0.05):
    rs = np.random.RandomState(seed)
    coarse = rs.randint(1, n_ids + 1, (ny // 3 + 1, nx // 3 + 1))
    ids = np.kron(coarse, np.ones((3, 3), np.int64))[:ny, :nx].astype(np.int32)
    flip = rs.rand(ny, nx)
    ids[flip < holes] = 0
    ids[(flip >= holes) & (flip < 2 * holes)] = rs.randint(1, n_ids + 1, int(((flip >= holes) & (flip < 2 * holes)).sum()))
    return ids


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_against_scipy_label(boundary):
    for seed, (ny, nx, n_ids) in enumerate(((20, 31, 3), (33, 17, 2), (48, 48, 5), (7, 90, 2))):
        ids = blobs(ny, nx, n_ids, seed)
        r = lc.label(ids=ids, boundary=boundary, max_sweeps=0)          # (no cleanup: the components themselves)
        want = scipy_partition(ids, boundary == "periodic")
        assert lc.same_partition(r["image"], want), (boundary, seed)
        assert r["status"]["n_components"] == len(np.unique(want[want > 0])) and r["status"]["n_unfilled"] == int((ids == 0).sum())


def test_golden_frames_in_ids_mode():
    g = golden()
    for t, frame in enumerate(g["frames"]):
        r = restated(("frame", t), ids=frame)
        present = len(np.unique(frame))
        assert r["status"]["n_components"] == present == r["n_grain"] and r["status"]["n_specks"] == 0, t   # no id lies in two pieces
        assert np.array_equal(r["image"], lc.relabel_by_first_pixel(frame)), t
    r = restated(("frame", 0), ids=g["frames"][0])
    assert r["n_grain"] == 118 and r["status"]["n_sweeps"] == 0 and np.array_equal(r["image"], g["clean"])
    v = vc.vectorize(r["image"], 118, "points")
    assert vc.is_valid(v["status"]) and v["status"]["n_joint"] == 236 and v["status"]["n_open_pairs"] == 0


def first_pixel_angles(g):
    """theta of the clean frame's grains in the labelling's numbering."""
    first = np.array([np.nonzero(g["clean"].reshape(-1) == k + 1)[0][0] for k in range(118)])
    return g["theta"][:, g["frames"][0].reshape(-1)[first] - 1]


def test_golden_frame_in_angles_mode():
    g = golden()
    r, _ = golden_restated("clean", "angles")
    assert np.array_equal(r["image"], g["clean"]) and r["n_grain"] == 118 and r["status"]["n_components"] == 118
    want = first_pixel_angles(g)
    assert r["mean_angles"].shape == (2, 118) and r["mean_angles"].dtype == np.float32
    assert np.abs(r["mean_angles"].astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -24
    # no two grains can fuse at tol = 1e-3: the smallest gap between two grains in the larger channel
    gap = np.abs(g["theta"][:, :, None] - g["theta"][:, None, :]).max(0) + np.eye(118) * 9
    assert gap.min() > 5e-3


@pytest.mark.parametrize("tag", sorted(NOISE))
def test_noise_on_the_golden_frame_reproduces_the_recorded_table(tag):
    g = golden()
    grains, sweeps, unfilled, differing = NOISE[tag]
    a, _ = golden_restated(tag, "ids")
    b, _ = golden_restated(tag, "angles")
    got = (a["n_grain"], a["status"]["n_sweeps"], a["status"]["n_unfilled"], int((a["image"] != g["clean"]).sum()))
    print(tag, got, a["status"])
    assert got == (grains, sweeps, unfilled, differing)
    assert np.array_equal(a["image"], b["image"]) and a["status"] == b["status"]
    v = vc.vectorize(a["image"], 118, "points")
    assert vc.is_valid(v["status"]) and v["status"]["n_joint"] == 236
    assert np.abs(b["mean_angles"].astype(np.float64) - first_pixel_angles(g).astype(np.float64)).max() <= 2.0 ** -24


def test_entry_point_validates_on_the_host():
    lib = _lib.load()
    assert lib.ggnn_version() == 26 == _lib.GGNN_ABI_VERSION and {"ggnn_label_grains", "ggnn_label_workspace_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    assert lib.ggnn_label_grains(None, None) == -1
    assert lib.ggnn_label_workspace_bytes(2, 8, 0) == 0 and lib.ggnn_label_workspace_bytes(8, 8, 5) == 0 and lib.ggnn_label_workspace_bytes(1 << 15, 8, 0) == 0
    need = lib.ggnn_label_workspace_bytes(32, 32, 2)
    assert need >= 32 * 32 * (21 + 16) and lib.ggnn_label_workspace_bytes(32, 32, 0) < need
    buf = (ctypes.c_int64 * 64)()                 # (host memory: refused before anything would be launched)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(**kw):
        A = _lib.LabelArgs(None, p, None, p, p, p, p, need, 32, 32, 64, 1, 0.001, 2, 4, 0)
        A.image = None                            # (so that a call that passes every other check still launches nothing)
        for k, v in kw.items():
            setattr(A, k, v)
        return lib.ggnn_label_grains(ctypes.byref(A), None)
    assert call() == -1
    for bad in (dict(ids=p), dict(angles=None), dict(status=None), dict(workspace=None), dict(mean_angles=None), dict(nx=2), dict(ny=2),
                dict(nx=1 << 15), dict(K=0), dict(K=5), dict(tol=-1.0), dict(tol=float("nan")), dict(min_pixels=0), dict(max_sweeps=-1),
                dict(max_sweeps=_lib.GGNN_LABEL_MAX_SWEEPS + 1), dict(grain_capacity=0), dict(grain_capacity=2 ** 31 - 1),
                dict(boundary=2), dict(status=p.value + 4), dict(workspace=p.value + 4), dict(mean_angles=p.value + 2),
                dict(workspace_bytes=need - 1), dict(angles=None, ids=p, K=2)):
        assert call(image=p, **bad) == -1, bad


def test_header_binding_and_struct_agree():
    import re
    src = open(os.path.join(ROOT, "include", "ggnn.h")).read()
    for name in ("GGNN_LABEL_TILE_X", "GGNN_LABEL_TILE_Y", "GGNN_LABEL_STATUS_WORDS", "GGNN_LABEL_MAX_SWEEPS"):
        assert f"#define {name} {getattr(_lib, name)}\n" in src, name
    body = re.search(r"typedef struct ggnn_label_args \{(.*?)\} ggnn_label_args;", src, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in _lib.LabelArgs._fields_]
    assert ctypes.sizeof(_lib.LabelArgs) == 8 * 8 + 4 * 8 + 4 * 4
    assert vz.LABEL_STATUS_WORDS == lc.STATUS and len(lc.STATUS) == _lib.GGNN_LABEL_STATUS_WORDS


def test_python_entry_points_refuse_what_they_cannot_take():
    host = torch.ones(8, 8, dtype=torch.int32)
    for kw, match in ((dict(), "exactly one"), (dict(ids=host, angles=host), "exactly one"), (dict(ids=host), "device"),
                      (dict(ids=host, boundary="open"), "boundary")):
        with pytest.raises(_lib.GGNNError, match=match):
            vz.label_grains(**kw)
    with pytest.raises(_lib.GGNNError, match="equal-shaped"):
        vz.sample_from_orientations(host, host[:4], 2.0, 0.4, 1e-3)


# ---- GPU: the kernels equal the restatement bit for bit ----------------------------------------------------------------------

def run(kw):
    """label_grains on the device for the restatement's keywords."""
    dev = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    if "tol" in dev:
        dev["tol"] = float(dev["tol"])
    return vz.label_grains(**dev)


def assert_equals_restatement(got, r, what):
    image, n_grain, means, status = got
    print(what, status)
    assert status == r["status"], (what, status, r["status"])
    assert status["n_bound_hits"] == 0 and n_grain == r["n_grain"], what
    assert image.dtype == torch.int32 and np.array_equal(image.cpu().numpy(), r["image"]), what
    if r["mean_angles"] is None:
        assert means is None, what
    else:
        assert means.dtype == torch.float32 and means.shape == r["mean_angles"].shape, what
        assert np.array_equal(means.cpu().numpy().view(np.uint32), r["mean_angles"].view(np.uint32)), what


def voronoi_map(ny, nx, boundary, seed, noise=0.01):
    """-> (ids, angles [2, ny, nx]): random Voronoi cells with `noise` of the pixels non-indexed or wrong, half each."""
    def make():
        rs = np.random.RandomState(seed)
        n = max(2, ny * nx // 150)
        ids = tk.voronoi([(rs.uniform(0, ny), rs.uniform(0, nx)) for _ in range(n)], ny, nx, periodic=boundary == "periodic")
        theta = f32(np.stack([np.linspace(0.05, 1.5, n)[rs.permutation(n)], np.linspace(1.5, 0.05, n)[rs.permutation(n)]]))
        m = rs.rand(ny, nx)
        if ny * nx <= 9:
            m[1, 1] = 0.0                             # (1 % of nine pixels: one, so that the sweeps run here too)
        ids[m < noise / 2] = 0
        wrong = (m >= noise / 2) & (m < noise)
        ids[wrong] = rs.randint(1, n + 1, int(wrong.sum()))
        angles = theta[:, np.maximum(ids, 1) - 1]
        angles[:, ids == 0] = np.nan
        return ids, np.ascontiguousarray(angles)
    return cached(("voronoi", ny, nx, boundary, seed), make)


SEAM_SHAPES = [(TY - 1, TX + 1), (TY, TX), (2 * TY + 1, 2 * TX - 1), (3, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("shape", SEAM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_that_place_seams(shape, boundary):
    ids, angles = voronoi_map(*shape, boundary, 11)
    for mp in (1, 3):
        for mode, kw in (("ids", dict(ids=ids)), ("angles", dict(angles=angles, tol=1e-3))):
            kw = dict(kw, min_pixels=mp, boundary=boundary)
            assert_equals_restatement(run(kw), restated(("seams", shape, boundary, mode, mp), **kw), (shape, boundary, mode, mp))


def serpentine(ny, nx, vertical=False, cut=None):
    """A path one pixel wide that fills every other row (column) and turns at alternating ends: one component whose pixels lie
    about ny nx / 2 links apart; cut: a turn left out."""
    if vertical:
        return np.ascontiguousarray(serpentine(nx, ny, cut=cut).T)
    img = np.zeros((ny, nx), np.int32)
    img[0::2] = 1
    for k, y in enumerate(range(1, ny - 1, 2)):
        if k != cut:
            img[y, nx - 1 if k % 2 == 0 else 0] = 1
    return img


def comb(ny, nx):
    img = np.zeros((ny, nx), np.int32)
    img[:, 0::2] = 1
    img[-1] = 1
    return img


def spiral(ny, nx):
    """A rectangular spiral one pixel wide from (0, 0) inwards, with its outer ring cut on the right wall: the first row and
    the stub below its end meet the rest only through the wrap (row 0 | row ny - 1, column 0 | column nx - 1)."""
    img = np.zeros((ny, nx), np.int32)
    y, x, dy, dx = 0, 0, 0, 1
    img[0, 0] = 1
    free = lambda a, b: 0 <= a < ny and 0 <= b < nx and img[a, b] == 0
    while True:
        for _ in range(2):
            if free(y + dy, x + dx) and (not (0 <= y + 2 * dy < ny and 0 <= x + 2 * dx < nx) or img[y + 2 * dy, x + 2 * dx] == 0):
                y, x = y + dy, x + dx
                img[y, x] = 1
                break
            dy, dx = dx, -dy
        else:
            break
    img[5, nx - 1] = 0
    return img


STRESS = {"serpentine along rows": lambda: serpentine(2 * TY + 1, 3 * TX + 1), "serpentine along columns": lambda: serpentine(2 * TY + 1, 3 * TX + 1, True),
          "comb": lambda: comb(2 * TY + 1, 3 * TX + 1), "spiral": lambda: spiral(2 * TY + 1, 3 * TX + 1),
          "serpentine cut in the middle": lambda: serpentine(2 * TY + 1, 3 * TX + 1, cut=8)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STRESS))
def test_union_find_stress_across_tiles(name):
    ids = STRESS[name]()
    for boundary in BOUNDARIES:
        kw = dict(ids=ids, boundary=boundary, max_sweeps=0)
        r = restated(("stress", name, boundary), **kw)
        if name in ("serpentine along rows", "serpentine along columns", "comb") or boundary == "periodic":
            assert r["status"]["n_components"] == 1 and r["status"]["n_unfilled"] == int((ids == 0).sum()), (name, boundary)
        else:
            assert r["status"]["n_components"] == 2, (name, boundary)      # closed through the wrap alone
        assert_equals_restatement(run(kw), r, (name, boundary))
    kw = dict(angles=f32(ids)[None] * np.float32(0.5) + np.float32(0.25), tol=0.01)    # the same in angles: 0.75 | 0.25
    r = restated(("stress", name, "angles"), **kw)
    assert r["status"]["n_components"] >= 2
    assert_equals_restatement(run(kw), r, (name, "angles"))


@pytest.mark.gpu
@pytest.mark.parametrize("boundary,shape", [("periodic", (TY, TX)), ("noflux", (TY - 1, TX + 1)), ("periodic", (2 * TY + 2, 2 * TX))])
def test_checkerboards(boundary, shape):
    ny, nx = shape
    ids = ((np.add.outer(np.arange(ny), np.arange(nx)) % 2) + 1).astype(np.int32)
    angles = f32(ids)[None] * np.float32(0.5)
    for kw in (dict(ids=ids), dict(angles=angles, tol=0.1), dict(ids=ids, grain_capacity=ny * nx // 2 + 3),
               dict(angles=angles, tol=0.1, grain_capacity=ny * nx // 2 + 3), dict(ids=ids, min_pixels=2)):
        kw = dict(kw, boundary=boundary)
        r = restated(("checkerboard", shape, boundary, tuple(sorted(k for k in kw)), kw.get("grain_capacity")), **kw)
        s = r["status"]
        if kw.get("min_pixels") == 2:
            assert s["n_unfilled"] == ny * nx and s["n_grains"] == 0 and s["n_specks"] == ny * nx and not r["image"].any()
        else:
            assert s["n_grains"] == ny * nx and s["overflow"] == (1 if "grain_capacity" in kw else 0)
            assert np.array_equal(r["image"].reshape(-1), np.arange(ny * nx) + (1 if boundary == "periodic" else 2))
        got = run(kw)
        assert_equals_restatement(got, r, (boundary, shape, sorted(kw)))
        if "grain_capacity" in kw and "angles" in kw:
            assert got[2].shape == (1, kw["grain_capacity"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_drawn_cases_on_the_device(name):
    kw, _ = HAND[name]
    assert_equals_restatement(run(kw), restated(("hand", name), **kw), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(WRAP))
def test_wrap_cases_on_the_device(name):
    ids = WRAP[name][0]
    for boundary in BOUNDARIES:
        assert_equals_restatement(run(dict(ids=ids, boundary=boundary)), restated(("wrap", name, boundary), ids=ids, boundary=boundary), (name, boundary))


GUARD = 64


def guarded_call(ids, angles, mask, tol, min_pixels, max_sweeps, boundary, cap):
    """The entry point itself with GUARD canary bytes or words before and after the image, the means, the status and the
    workspace -> (image, means, status) with their guards, and whether the workspace's guards survived."""
    lib = _lib.load()
    K, (ny, nx) = (0, ids.shape) if angles is None else (angles.shape[0], angles.shape[1:])
    need = lib.ggnn_label_workspace_bytes(nx, ny, K)
    image = torch.full((ny * nx + 2 * GUARD,), -7, dtype=torch.int32, device=DEV)
    means = torch.full((max(K, 1) * cap + 2 * GUARD,), -7.0, dtype=torch.float32, device=DEV)
    status = torch.full((9 + 2 * GUARD,), -7, dtype=torch.int64, device=DEV)
    ws = torch.full((need + 2 * 256,), 0x5A, dtype=torch.uint8, device=DEV)
    d_ids = None if ids is None else torch.from_numpy(ids).to(DEV)
    d_ang = None if angles is None else torch.from_numpy(np.ascontiguousarray(angles)).to(DEV)
    d_mask = None if mask is None else torch.from_numpy(mask.astype(np.uint8)).to(DEV)
    A = _lib.LabelArgs(_lib.ptr(d_ids), _lib.ptr(d_ang), _lib.ptr(d_mask), image[GUARD:].data_ptr(), means[GUARD:].data_ptr() if K else None,
                       status[GUARD:].data_ptr(), ws[256:].data_ptr(), need, nx, ny, cap, min_pixels, float(np.float32(tol or 0)), K,
                       max_sweeps, vz.BOUNDARIES[boundary])
    _lib.check(lib.ggnn_label_grains(ctypes.byref(A), _lib.current_stream()), "ggnn_label_grains")
    torch.cuda.synchronize()
    return image, means, status, bool((ws[:256] == 0x5A).all()) and bool((ws[256 + need:] == 0x5A).all())


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_guarded_arrays_and_a_capacity_inside_the_grains(boundary):
    ny, nx = 2 * TY + 1, 2 * TX - 1
    ids, angles = voronoi_map(ny, nx, boundary, 11)
    mask = np.ones((ny, nx), np.uint8)
    mask[3:6, 60:70] = 0
    for mode in ("ids", "angles"):
        full = lc.label(ids=ids, valid=mask, min_pixels=3, boundary=boundary)
        for cap in (full["n_grain"] - 2, full["n_grain"] + 5):
            kw = dict(ids=ids) if mode == "ids" else dict(angles=angles, tol=1e-3)
            r = lc.label(valid=mask, min_pixels=3, boundary=boundary, grain_capacity=cap, **kw)
            image, means, status, ws_ok = guarded_call(kw.get("ids"), kw.get("angles"), mask, kw.get("tol"), 3, 64, boundary, cap)
            assert ws_ok and dict(zip(lc.STATUS, status[GUARD:GUARD + 9].tolist())) == r["status"], (mode, cap)
            assert r["status"]["overflow"] == int(cap < full["n_grain"])
            assert bool((status[:GUARD] == -7).all()) and bool((status[GUARD + 9:] == -7).all())
            assert bool((image[:GUARD] == -7).all()) and bool((image[GUARD + ny * nx:] == -7).all())
            assert np.array_equal(image[GUARD:GUARD + ny * nx].cpu().numpy(), r["image"].reshape(-1))
            if mode == "ids":
                assert bool((means == -7).all())
                continue
            n = min(cap, r["n_grain"])
            rows_ = means[GUARD:GUARD + 2 * cap].view(2, cap)
            assert np.array_equal(rows_[:, :n].cpu().numpy().view(np.uint32), r["mean_angles"].view(np.uint32))
            assert bool((rows_[:, n:] == -7).all()) and bool((means[:GUARD] == -7).all()) and bool((means[GUARD + 2 * cap:] == -7).all())


@pytest.mark.gpu
def test_two_runs_and_a_captured_graph_give_the_same_bits():
    ny, nx = 2 * TY + 1, 2 * TX - 1
    ids, angles = voronoi_map(ny, nx, "periodic", 11)
    r = restated(("seams", (ny, nx), "periodic", "angles", 3), angles=angles, tol=1e-3, min_pixels=3, boundary="periodic")
    dev = torch.from_numpy(angles).to(DEV)
    args = (None, dev, 1e-3, None, 3, 64, "periodic", None)
    first, second = vz._label(*args), vz._label(*args)                  # (also the warm-up of the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = vz._label(*args)
    for _ in range(2):                                                  # (a replay starts from its own zeroed words)
        graph.replay()
    torch.cuda.synchronize()
    for k in ("image", "means", "status"):
        assert torch.equal(first[k], second[k]) and torch.equal(first[k], held[k]), k
    assert dict(zip(lc.STATUS, held["status"].tolist())) == r["status"] and np.array_equal(held["image"].cpu().numpy(), r["image"])


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["clean"] + sorted(NOISE), ids=str)
def test_golden_frame_end_to_end(tag):
    for mode in ("ids", "angles"):
        r, kw = golden_restated(tag, mode)
        assert_equals_restatement(run(kw), r, (tag, mode))


def assert_same_sample(a, b):
    for da, db in zip(a, b):
        assert da.keys() == db.keys()
        for k in da:
            assert da[k].dtype == db[k].dtype and torch.equal(da[k], db[k]), k


@pytest.mark.gpu
@torch.no_grad()
def test_sample_from_orientations_periodic_and_ten_rollout_steps():
    from graingraphnn_amd import GrainRollout
    g = golden()
    _, angles, mp = golden_inputs((0.04, 1))
    r, _ = golden_restated((0.04, 1), "angles")
    dev = torch.from_numpy(angles).to(DEV)
    kw = dict(span=6, patch_pixels=501 ** 2, grid="points")
    X, EI, EA, image, status = vz.sample_from_orientations(dev[0], dev[1], g["G"], g["R"], 1e-3, min_pixels=mp, **kw)
    assert np.array_equal(image.cpu().numpy(), r["image"]) and {k: status[k] for k in lc.STATUS} == r["status"]
    assert np.array_equal(np.stack([status["theta_x"], status["theta_z"]]).view(np.uint32), r["mean_angles"].view(np.uint32))
    assert_same_sample((X, EI, EA), vz.sample_from_image(image, status["theta_x"], status["theta_z"], g["G"], g["R"], **kw))
    assert X["grain"].shape == (118, 11) and X["joint"].shape == (236, 8) and int((EI[EDGE_TYPES[2]] < 0).sum()) == 0
    R, Cm = product_models(10020, 1.0, DEV)
    ro = GrainRollout(R, Cm, X, EI, EA, 6, refresh_centres=True)
    for _ in range(10):
        pred = ro.step()
        assert all(bool(torch.isfinite(t).all()) for t in pred.values())
    assert not ro.range_exceeded()


@pytest.mark.gpu
@torch.no_grad()
def test_sample_from_orientations_on_the_noflux_golden():
    d = np.load(os.path.join(GOLDEN, "grain_image_cfg1.npz"))
    # the record's phase-field image of the no-flux run holds nothing: every pixel is non-indexed and stays unfilled
    empty = d["noflux__alpha_pde"].astype(np.int32)
    assert not empty.any()
    image, n_grain, means, status = vz.label_grains(ids=torch.from_numpy(empty).to(DEV), boundary="noflux")
    assert n_grain == 1 and status["n_unfilled"] == 501 * 501 == status["n_invalid_in"] and not bool(image.any()) and means is None
    nan = torch.full((501, 501), float("nan"), device=DEV)
    with pytest.raises(ValueError, match="not a valid noflux"):
        vz.sample_from_orientations(nan, nan, 2.0, 0.5, 1e-3, boundary="noflux", span=6)
    # the structure itself: ids 2 .. 101, per-grain angles from a seeded draw
    field = d["noflux__alpha_field"].astype(np.int32)
    rs = np.random.RandomState(7)
    theta = f32(np.stack([rs.uniform(0, np.pi / 2, 102), rs.uniform(0, np.pi / 2, 102)]))
    angles = theta[:, field]
    r = restated("noflux golden", angles=angles, tol=1e-4, boundary="noflux")
    assert r["n_grain"] == 101 and np.array_equal(r["image"], lc.relabel_by_first_pixel(field) + 1)
    v = vn.vectorize(r["image"], 101, "points")
    assert vn.is_valid(v["status"]) and v["status"]["n_joint"] == 198
    dev = torch.from_numpy(angles).to(DEV)
    kw = dict(span=6, patch_pixels=501 ** 2, grid="points", boundary="noflux")
    X, EI, EA, image, status = vz.sample_from_orientations(dev[0], dev[1], 2.0, 0.5, 1e-4, **kw)
    assert np.array_equal(image.cpu().numpy(), r["image"]) and {k: status[k] for k in lc.STATUS} == r["status"]
    assert np.array_equal(np.stack([status["theta_x"], status["theta_z"]]).view(np.uint32), r["mean_angles"].view(np.uint32))
    assert status["theta_x"][0] == 0 and status["theta_z"][0] == 0
    assert_same_sample((X, EI, EA), vz.sample_from_image(image, status["theta_x"], status["theta_z"], 2.0, 0.5, **kw))
    assert X["grain"].shape == (101, 11) and X["joint"].shape == (198, 8)
