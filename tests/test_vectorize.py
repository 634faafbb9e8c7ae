"""A rollout's first state from a grain-ID image (ggnn_image_junctions / ggnn_junction_links, graingraphnn_amd.vectorize)
against the numpy restatement of tests/vectorcheck.py, and the restatement against the reference's own data.

The contract.  KERNELS against RESTATEMENT: every output array and every status word equal, bit for bit.  RESTATEMENT
against the REFERENCE: on the phase-field frame 0 of seed 10020 (grain_image_cfg1.npz, `init__alpha_pde`) the junction
triples are graph_40.npz's, the joint->joint pairs its 354, the area feature its x_grain[:, 3] bit for bit, and every
coordinate lies within half a grid step of its own.  On rasters of the fixtures' polygons (rastercheck.grain_image) a triple
may differ from the graph's only inside a counted quadruple window.

ROUND TRIP: vectorise an image, restate the polygons (polycheck.restate, fp32), rasterise them (rastercheck.grain_image):
the share of pixels that differ from the input, measured here with the restatement,
  init 501^2 0.028797   graph_40 at 256 0.041580   at 128 0.082764   at 96 0.109809   graph_120 at 1024 0.031427
  generated_80_seed7 at 512 0.043667
is capped at the measured value plus a quarter (polygons with straight sides cannot follow a pixel boundary closer)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import polycheck as pc
import rastercheck as rc
import vectorcheck as vc
from helpers import GOLDEN, product_models
from graingraphnn_amd import _lib
from graingraphnn_amd import vectorize as vz
from graingraphnn_amd.synthetic import EDGE_TYPES

DEV = "cuda"
U32 = 2.0 ** -24
# Both sides of a coordinate comparison are fp32 numbers below 2: the position carries three roundings (the pitch, the sum,
# the product; xr + off and the quotients that occur are exact or rounded once more), the reference's value one.
FP32_ROOM = 4 * 2 * U32
MEASURED_ROUND_TRIP = {"init": 0.02879669802112342, "graph_40@256": 0.0415802001953125, "graph_40@128": 0.082763671875,
                       "graph_40@96": 0.10980902777777778, "graph_120@1024": 0.03142738342285156,
                       "generated_80_seed7@512": 0.043666839599609375}


def npz(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def reference_triples(d):
    """The sorted grain triple of every junction of a fixture graph, by junction."""
    t = {}
    for g, j in d["ei_grain__push__joint"].T:
        t.setdefault(int(j), []).append(int(g))
    assert sorted(t) == list(range(d["x_joint"].shape[0]))
    return [tuple(sorted(t[j])) for j in range(len(t))]


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def fixture_raster(name, s):
    """The fixture graph's polygons (restated) filled into an s x s image, computed once."""
    def make():
        d = npz(name)
        rowptr, col = pc.table_of(d["ei_joint__pull__grain"], d["x_grain"].shape[0])
        img = rc.grain_image(rowptr, pc.restate(rowptr, col, d["x_joint"])["xy_sorted"], (s, s))
        img.setflags(write=False)
        return img
    return cached((name, s), make)


def pde_image(tag="init"):
    return cached(("pde", tag), lambda: npz("grain_image_cfg1")[tag + "__alpha_pde"].astype(np.int32))


def restated(key, image, n_grain, grid="cells", **kw):
    """The restatement of a named image, computed once and left unchanged."""
    return cached(("restated", key, grid, tuple(sorted(kw.items()))), lambda: vc.vectorize(image, n_grain, grid, **kw))


def round_trip(v, image, n_grain):
    """(share of differing pixels, the image) of the polygons of a vectorised image, rasterised again."""
    xj = np.zeros((len(v["xy"]), 8), np.float32)
    xj[:, :2] = v["xy"]
    rowptr, col = pc.table_of(v["gj"][::-1], n_grain)
    out = rc.grain_image(rowptr, pc.restate(rowptr, col, xj)["xy_sorted"], (image.shape[1], image.shape[0]))
    return float((out != image).mean()), out


def check_round_trip(key, v, image, n_grain):
    share, _ = cached(("round trip", key), lambda: round_trip(v, image, n_grain))
    print(f"{key}: round-trip share {share!r}")
    assert share <= 1.25 * MEASURED_ROUND_TRIP[key], (key, share)


def periodic_gap(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return np.minimum(d, np.abs(1.0 - d))


# ---- CPU: the restatement against the reference's data ---------------------------------------------------------------------

def test_phase_field_frame_0_gives_the_reference_graph():
    g40, image = npz("graph_40"), pde_image()
    v = restated("init", image, 118, "points")
    s = v["status"]
    assert vc.is_valid(s) and s["n_joint"] == 236 and s["n_quad_windows"] == 0, s
    ref = reference_triples(g40)
    got = [tuple(t) for t in v["triples"].tolist()]
    assert len(set(ref)) == 236 and set(got) == set(ref) and len(got) == 236
    at = {t: j for j, t in enumerate(ref)}
    to_ref = np.array([at[t] for t in got])
    pairs = {tuple(sorted((int(to_ref[a]), int(to_ref[b])))) for a, b in v["jj"].T}
    want = {tuple(sorted((int(a), int(b)))) for a, b in g40["ei_joint__connect__joint"].T}
    assert len(want) == 354 and pairs == want
    gap = periodic_gap(v["xy"], g40["x_joint"][to_ref, :2])
    print(f"largest coordinate gap {gap.max() * 500:.6f} grid steps")
    assert gap.max() <= 0.5 / 500 + FP32_ROOM, gap.max() * 500
    counts = rc.compare(image, None, 118)[1][1:]
    area = (counts / 501 ** 2).astype(np.float32)
    assert np.array_equal(area.view(np.uint32), g40["x_grain"][:, 3].view(np.uint32))
    check_round_trip("init", v, image, 118)


@pytest.mark.parametrize("tag", ["step1", "step3", "mass3"])
def test_later_phase_field_frames_are_valid(tag):
    s = restated(tag, pde_image(tag), 118, "points")["status"]
    assert vc.is_valid(s) and s["n_joint"] == 236, (tag, s)


@pytest.mark.parametrize("size,quads", [(96, 1), (128, 1), (256, 0)])
def test_rasters_of_graph_40_give_its_triples(size, quads):
    g40, image = npz("graph_40"), fixture_raster("graph_40", size)
    v = restated(("graph_40", size), image, 118)
    s = v["status"]
    assert vc.is_valid(s) and s["n_quad_windows"] == quads, s
    ref = reference_triples(g40)
    got = [tuple(t) for t in v["triples"].tolist()]
    assert set(got) == set(ref) and len(got) == len(ref)            # 0 missing, 0 spurious
    at = {t: j for j, t in enumerate(ref)}
    gap = periodic_gap(v["xy"], g40["x_joint"][[at[t] for t in got], :2])
    print(f"graph_40 at {size}: largest coordinate gap {gap.max() * size:.6f} pixels")
    assert gap.max() <= 1.0 / size + FP32_ROOM, gap.max() * size    # (the vertex is truncated to its pixel)
    check_round_trip(f"graph_40@{size}", v, image, 118)


def test_raster_of_graph_120_differs_inside_quadruples_only():
    g120, image = npz("graph_120"), fixture_raster("graph_120", 1024)
    v = restated(("graph_120", 1024), image, 1043)
    assert vc.is_valid(v["status"]) and v["status"]["n_joint"] == 2086, v["status"]
    got, ref = {tuple(t) for t in v["triples"].tolist()}, set(reference_triples(g120))
    print(f"graph_120 at 1024: missing {len(ref - got)}, spurious {len(got - ref)}, quadruples {v['quads']}")
    assert len(v["quads"]) == v["status"]["n_quad_windows"]
    for t in got ^ ref:
        assert any(set(t) <= set(q) for q in v["quads"]), t
    check_round_trip("graph_120@1024", v, image, 1043)


def test_round_trip_of_generated_80():
    image = fixture_raster("generated_80_seed7", 512)
    n_grain = npz("generated_80_seed7")["x_grain"].shape[0]
    v = restated(("generated_80_seed7", 512), image, n_grain)
    assert vc.is_valid(v["status"]), v["status"]
    check_round_trip("generated_80_seed7@512", v, image, n_grain)


def test_sub_pixel_edges_are_reported_not_repaired():
    """generated_40_seed1 at 256: edges shorter than a pixel leave a raster that is no valid structure, and the status says so."""
    image = fixture_raster("generated_40_seed1", 256)
    v = restated(("generated_40_seed1", 256), image, 115)
    s = v["status"]
    assert s["n_open_pairs"] > 0 and s["n_joint"] != 2 * s["n_present_grains"] and not vc.is_valid(s), s
    assert int((v["jj"][1] == -1).sum()) == s["n_open_pairs"] and s["n_present_grains"] == 115


# ---- hand-made images -----------------------------------------------------------------------------------------------------

def bricks(ny, nx, row_edges, cuts):
    """Rows r = [row_edges[r], row_edges[r + 1]) (the last one wraps round to row_edges[0]); in row r a brick begins at
    every x of cuts[r] (the last one wraps round).  -> (int32 [ny, nx] of ids from 1, the number of bricks)."""
    img, gid = np.zeros((ny, nx), np.int32), 0
    for r, c in enumerate(cuts):
        y0, y1 = row_edges[r], row_edges[(r + 1) % len(cuts)]
        ys = [y % ny for y in range(y0, y1 if y1 > y0 else y1 + ny)]
        for i, x0 in enumerate(c):
            x1 = c[(i + 1) % len(c)]
            gid += 1
            img[np.ix_(ys, [x % nx for x in range(x0, x1 if x1 > x0 else x1 + nx)])] = gid
    return img, gid


def brick_cases():
    """name -> (image, n_grain, keywords of the restatement, what the status must show)."""
    even, odd = [0, 8, 16, 24], [4, 12, 20, 28]
    plain, n = bricks(32, 32, [0, 8, 16, 24], [even, odd, even, odd])
    quad, _ = bricks(32, 32, [0, 8, 16, 24], [even, [4, 16, 20, 28], even, odd])      # rows 0 and 1 both cut at x = 16
    diagonal = plain.copy()                        # the junction of bricks 2 | 5, 6 at (y, x) = (8, 12), its boundary stepped
    diagonal[8, 13], diagonal[9, 12] = plain[7, 13], plain[8, 11]
    sliver = plain.copy()
    sliver[8:14, 9] = plain[8, 12]                 # a line of brick 6 inside brick 5, under brick 2: (1, 4, 5) twice at radius 1
    invalid = plain.copy()
    invalid[3, 3], invalid[8, 12], invalid[20, 5] = 0, n + 1, -4
    rect, n_rect = bricks(17, 33, [0, 6, 12], [[0, 11, 22], [5, 16, 27], [8, 19, 30]])
    seam = np.roll(np.roll(diagonal, -8, 0), -12, 1)   # the stepped junction's windows at (31, 31) and (0, 0)
    valid = dict(valid=True, n_merged_windows=0, n_quad_windows=0)
    return {
        "plain": (plain, n, {}, dict(valid, n_joint=32)),
        "plain, points grid": (plain, n, dict(grid="points"), dict(valid, n_joint=32)),
        "quadruple": (quad, n, {}, dict(valid=True, n_quad_windows=2, n_joint=32)),
        "diagonal": (diagonal, n, {}, dict(valid=True, n_merged_windows=1, n_joint=32)),
        "diagonal, radius 0": (diagonal, n, dict(merge_radius=0), dict(valid=False, n_merged_windows=0, n_joint=33)),
        "diagonal, radius 1": (diagonal, n, dict(merge_radius=1), dict(valid=True, n_merged_windows=1)),
        "triple twice": (sliver, n, dict(merge_radius=1), dict(valid=False, n_invalid_pixels=0, overflow=0, n_joint=33)),
        "invalid pixels": (invalid, n, {}, dict(valid=False, n_invalid_pixels=3)),
        "33 x 17": (rect, n_rect, {}, dict(valid, n_joint=18, n_present_grains=9)),
        "seam": (seam, n, {}, dict(valid=True, n_merged_windows=1, n_joint=32)),
        "capacity one short": (plain, n, dict(joint_capacity=31), dict(valid=False, overflow=1, n_joint=32)),
        "capacity to spare": (plain, n, dict(joint_capacity=20000), dict(valid, n_joint=32)),   # (its table stays cheap)
    }


CASE_NAMES = ("plain", "plain, points grid", "quadruple", "diagonal", "diagonal, radius 0", "diagonal, radius 1", "triple twice",
              "invalid pixels", "33 x 17", "seam", "capacity one short", "capacity to spare")


def case(name):
    """A hand-made image by name, built on first use."""
    cases = cached("bricks", brick_cases)
    assert tuple(cases) == CASE_NAMES
    return cases[name]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_on_hand_made_images(name):
    """The hand-made images show what they were made for (the GPU tests below run the kernels on the same ones)."""
    image, n_grain, kw, want = case(name)
    assert image.shape[0] <= 33 and image.shape[1] <= 33
    v = restated(("brick", name), image, n_grain, **kw)
    s = dict(v["status"], valid=vc.is_valid(v["status"]))
    assert {k: s[k] for k in want} == want, (name, s)
    triples = [tuple(t) for t in v["triples"].tolist()]
    if name == "triple twice":
        assert len(set(triples)) == len(triples) - 1 and s["n_open_pairs"] > 0
    elif name not in ("diagonal, radius 0",):
        assert len(set(triples)) == len(triples)                     # no triple repeats
    if name == "seam":   # the merged junction sits on the seam: its representative is the window (0, 0), not (31, 31)
        assert (v["xy"] > 1.0).sum() == 0 and np.any(np.all(v["xy"] == np.float32(0.5) * np.float32(1 / 32), axis=1))
    if name == "capacity one short":
        assert len(v["xy"]) == 31 and v["gj"].shape == (2, 93)


def test_positions_follow_the_stated_order_of_operations():
    """One junction of three carriers: x = ((float)xr + off + Sx / m) * pitch with every step rounded to fp32."""
    image, n_grain, _, _ = case("diagonal")
    f = np.float32
    for grid in ("cells", "points"):
        v = vc.vectorize(image, n_grain, grid)
        off, pitch = vc.grid_constants(32, grid)
        j = [tuple(t) for t in v["triples"].tolist()].index((1, 4, 5))
        want = f(f(f(11) + off) + f(f(1) / f(2))) * pitch, f(f(f(7) + off) + f(f(1) / f(2))) * pitch
        assert v["xy"][j].tolist() == [float(want[0]), float(want[1])], (grid, v["xy"][j], want)


def test_entry_points_validate_on_the_host():
    lib = _lib.load()
    assert lib.ggnn_version() == 26 == _lib.GGNN_ABI_VERSION
    assert {"ggnn_image_junctions", "ggnn_junction_links"} <= set(_lib.EXPORTED_SYMBOLS)
    assert ctypes.sizeof(_lib.JunctionArgs) == 8 * 8 + 4 * 8 + 4 * 4 and ctypes.sizeof(_lib.LinkArgs) == 5 * 8 + 3 * 8
    assert lib.ggnn_image_junctions(None, None) == -1 and lib.ggnn_junction_links(None, None) == -1
    buf = (ctypes.c_int64 * 64)()                 # (host memory: refused before anything would be launched)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def jargs(**kw):
        A = _lib.JunctionArgs(p, p, p, p, p, p, p, 4 * 64, 32, 32, 16, 8, 1.0, 1.0 / 32, 2, 0)
        for k, v in kw.items():
            setattr(A, k, v)
        return ctypes.byref(A)
    for bad in (dict(image=None), dict(pixel_counts=None), dict(xy=None), dict(triples=None), dict(edge_gj=None),
                dict(status=None), dict(workspace=None), dict(status=p.value + 4), dict(edge_gj=p.value + 4),
                dict(merge_radius=-1), dict(merge_radius=8), dict(nx=4), dict(ny=4), dict(nx=1 << 15), dict(ny=1 << 15),
                dict(n_grain=0), dict(n_grain=2 ** 31 - 2), dict(joint_capacity=0), dict(joint_capacity=2 ** 31 // 3 + 1),
                dict(offset=-0.5), dict(offset=2.0), dict(pitch=0.0), dict(pitch=float("nan")), dict(pitch=1.5),
                dict(workspace_bytes=4 * 32 - 1), dict(nx=257, workspace_bytes=4 * 64 - 1)):
        assert lib.ggnn_image_junctions(jargs(**bad), None) == -1, bad

    def largs(**kw):
        A = _lib.LinkArgs(p, p, p, p, p, 16, 8, 24)
        for k, v in kw.items():
            setattr(A, k, v)
        return ctypes.byref(A)
    for bad in (dict(triples=None), dict(rowptr=None), dict(col=None), dict(edge_jj=None), dict(status=None),
                dict(status=p.value + 4), dict(edge_jj=p.value + 4), dict(n_grain=0), dict(joint_capacity=0), dict(E_cap=-1),
                dict(E_cap=2 ** 31 - 1)):
        assert lib.ggnn_junction_links(largs(**bad), None) == -1, bad


def test_python_entry_points_refuse_what_they_cannot_take():
    with pytest.raises(_lib.GGNNError, match="device tensor"):
        vz.graph_from_image(torch.ones(8, 8, dtype=torch.int32), n_grain=1)
    assert vz.status_is_valid(dict(zip(vz.STATUS_WORDS, (4, 1, 0, 0, 0, 2, 0))))
    for word in ("n_invalid_pixels", "n_open_pairs", "overflow", "n_joint"):
        s = dict(zip(vz.STATUS_WORDS, (4, 1, 0, 0, 0, 2, 0)))
        s[word] += 1
        assert not vz.status_is_valid(s), word
    assert vz.STATUS_WORDS == vc.STATUS


# ---- GPU: the kernels equal the restatement bit for bit --------------------------------------------------------------------

def assert_equals_restatement(got, v, what):
    """got = graph_from_image's (xy, triples, edge_index_dict, status)."""
    xy, triples, ei, status = got
    assert status == v["status"], (what, status, v["status"])
    assert xy.dtype == torch.float32 and triples.dtype == torch.int32 and all(ei[et].dtype == torch.int64 for et in EDGE_TYPES)
    assert np.array_equal(triples.cpu().numpy(), v["triples"]), what
    assert np.array_equal(xy.cpu().numpy().view(np.uint32), v["xy"].view(np.uint32)), what
    assert np.array_equal(ei[EDGE_TYPES[0]].cpu().numpy(), v["gj"]), what
    assert np.array_equal(ei[EDGE_TYPES[1]].cpu().numpy(), v["gj"][::-1]), what
    assert np.array_equal(ei[EDGE_TYPES[2]].cpu().numpy(), v["jj"]), what
    assert all(ei[et].is_contiguous() for et in EDGE_TYPES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_kernels_against_the_restatement_on_hand_made_images(name):
    image, n_grain, kw, _ = case(name)
    v = restated(("brick", name), image, n_grain, **kw)
    got = vz.graph_from_image(torch.from_numpy(image).to(DEV), n_grain=n_grain, strict=False, **kw)
    assert_equals_restatement(got, v, name)
    if vc.is_valid(v["status"]):
        assert_equals_restatement(vz.graph_from_image(torch.from_numpy(image).to(DEV), n_grain, **kw), v, name)
    else:
        with pytest.raises(ValueError, match="n_open_pairs"):
            vz.graph_from_image(torch.from_numpy(image).to(DEV), n_grain, **kw)


@pytest.mark.gpu
def test_nothing_is_written_beyond_the_capacity_or_the_junctions():
    """The two entry points themselves on guarded arrays: capacity one short of the 32 junctions, then four to spare.  The
    links and scan kernels share their code with the stack form, which writes joint_off behind the status rows: the four
    words behind the one row keep their guard through both calls."""
    image, n_grain, _, _ = case("plain")
    lib, dev_image = _lib.load(), torch.from_numpy(image).to(DEV)
    from graingraphnn_amd.backend import default_backend
    counts = default_backend().image_compare(dev_image, None, n_grain)[1]
    for cap in (31, 36):
        v = restated(("brick", "plain", cap), image, n_grain, joint_capacity=cap)
        n = min(cap, 32)
        xy = torch.full((2 * cap + 16,), -7.0, dtype=torch.float32, device=DEV)
        triples = torch.full((3 * cap + 16,), -7, dtype=torch.int32, device=DEV)
        gj = torch.full((6 * cap + 16,), -7, dtype=torch.int64, device=DEV)
        status = torch.full((7 + 4,), -7, dtype=torch.int64, device=DEV)
        ws = torch.empty(32, dtype=torch.int32, device=DEV)
        A = _lib.JunctionArgs(dev_image.data_ptr(), counts.data_ptr(), xy.data_ptr(), triples.data_ptr(), gj.data_ptr(),
                              status.data_ptr(), ws.data_ptr(), 4 * 32, 32, 32, n_grain, cap, 1.0, float(np.float32(1) / np.float32(32)),
                              2, 0)
        _lib.check(lib.ggnn_image_junctions(ctypes.byref(A), _lib.current_stream()), "ggnn_image_junctions")
        assert dict(zip(vc.STATUS, status[:7].tolist())) == dict(v["status"], n_open_pairs=0) and bool((status[7:] == -7).all())
        assert np.array_equal(xy[:2 * n].cpu().numpy().view(np.uint32), v["xy"].reshape(-1).view(np.uint32))
        assert np.array_equal(triples[:3 * n].cpu().numpy(), v["triples"].reshape(-1))
        assert bool((xy[2 * n:] == -7).all()) and bool((triples[3 * n:] == -7).all())
        rows = gj[:6 * cap].view(2, 3 * cap)
        assert np.array_equal(rows[:, :3 * n].cpu().numpy(), v["gj"])
        assert bool((rows[:, 3 * n:] == -7).all()) and bool((gj[6 * cap:] == -7).all())
        # ggnn_junction_links on the same guarded status, the table built as _vectorize builds it (spare rows past n)
        slots = torch.arange(cap, dtype=torch.int64, device=DEV).repeat_interleave(3)
        table = torch.stack([slots + n_grain, slots])
        table[:, :3 * n] = rows[:, :3 * n]
        csr = default_backend().build_csr_batch([(table.flip(0).contiguous(), cap, n_grain + cap)], check=False)[0]
        jj = torch.full((6 * cap + 16,), -7, dtype=torch.int64, device=DEV)
        L = _lib.LinkArgs(triples.data_ptr(), csr.rowptr.data_ptr(), csr.col.data_ptr(), jj.data_ptr(), status.data_ptr(),
                          n_grain, cap, csr.col.numel())
        _lib.check(lib.ggnn_junction_links(ctypes.byref(L), _lib.current_stream()), "ggnn_junction_links")
        assert dict(zip(vc.STATUS, status[:7].tolist())) == v["status"] and bool((status[7:] == -7).all())
        cols = jj[:6 * cap].view(2, 3 * cap)
        assert np.array_equal(cols[:, :3 * n].cpu().numpy(), v["jj"])
        assert bool((cols[:, 3 * n:] == -7).all()) and bool((jj[6 * cap:] == -7).all())


@pytest.mark.gpu
@pytest.mark.parametrize("size", [96, 256])
def test_kernels_on_rasters_of_graph_40(size):
    """236 junctions over many row segments: the scan crosses block boundaries (256: one segment a row, 96: a short one)."""
    image = fixture_raster("graph_40", size)
    v = restated(("graph_40", size), image, 118)
    assert_equals_restatement(vz.graph_from_image(torch.from_numpy(image.copy()).to(DEV), 118), v, size)
    # n_grain=None reads the largest id; an int64 image is taken as it is
    assert_equals_restatement(vz.graph_from_image(torch.from_numpy(image.astype(np.int64)).to(DEV)), v, (size, "int64"))


@pytest.mark.gpu
def test_sub_pixel_edges_through_the_device_path():
    image = fixture_raster("generated_40_seed1", 256)
    v = restated(("generated_40_seed1", 256), image, 115)
    dev_image = torch.from_numpy(image.copy()).to(DEV)
    with pytest.raises(ValueError, match="n_open_pairs"):
        vz.graph_from_image(dev_image, 115)
    got = vz.graph_from_image(dev_image, 115, strict=False)
    assert_equals_restatement(got, v, "generated_40_seed1")
    assert int((got[2][EDGE_TYPES[2]][1] == -1).sum()) == v["status"]["n_open_pairs"] > 0
    with pytest.raises(ValueError, match="n_open_pairs"):
        vz.sample_from_image(dev_image, np.zeros(115), np.zeros(115), 2.0, 0.4, span=6, strict=False)


@pytest.mark.gpu
def test_captured_graph_gives_the_same_bits():
    image, n_grain, _, _ = case("seam")
    v = restated(("brick", "seam"), image, n_grain)
    dev_image = torch.from_numpy(image).to(DEV)
    eager = vz._vectorize(dev_image, n_grain, "cells", 2, None)        # (also the warm-up of the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = vz._vectorize(dev_image, n_grain, "cells", 2, None)
    for _ in range(2):                                                  # (a replay starts from its own zeroed status)
        graph.replay()
    torch.cuda.synchronize()
    for k in ("xy", "triples", "gj", "jj", "status"):
        assert torch.equal(held[k], eager[k]), k
    assert dict(zip(vc.STATUS, held["status"].tolist())) == v["status"]
    assert np.array_equal(held["xy"][:32].cpu().numpy().view(np.uint32), v["xy"].view(np.uint32))


@pytest.mark.gpu
@torch.no_grad()
def test_phase_field_frame_0_into_a_rollout():
    """sample_from_image on the reference's 501 x 501 frame 0: the restatement's graph, the generator's layout; GrainRollout
    takes it as it is, and layer 0's grain image differs from the input by exactly the restated round-trip share."""
    from graingraphnn_amd import GrainRollout
    from graingraphnn_amd.generator import feature_rows
    g40, image = npz("graph_40"), pde_image()
    v = restated("init", image, 118, "points")
    rs = np.random.RandomState(3)
    theta_x, theta_z = rs.uniform(0, np.pi / 2, 118), rs.uniform(0, np.pi / 2, 118)
    dev_image = torch.from_numpy(image).to(DEV)
    X, EI, EA = vz.sample_from_image(dev_image, theta_x, theta_z, 2.0, 0.4, span=6, patch_pixels=501 ** 2, grid="points")
    assert {k: (tuple(t.shape), t.dtype) for k, t in X.items()} == {"grain": ((118, 11), torch.float32),
                                                                    "joint": ((236, 8), torch.float32)}
    assert np.array_equal(EI[EDGE_TYPES[0]].cpu().numpy(), v["gj"]) and np.array_equal(EI[EDGE_TYPES[2]].cpu().numpy(), v["jj"])
    assert np.array_equal(EI[EDGE_TYPES[1]].cpu().numpy(), v["gj"][::-1])
    xg, xj = X["grain"].cpu().numpy(), X["joint"].cpu().numpy()
    assert np.array_equal(xj[:, :2].view(np.uint32), v["xy"].view(np.uint32))
    assert np.array_equal(xg[:, 3].view(np.uint32), g40["x_grain"][:, 3].view(np.uint32))          # the reference's areas
    fg, fj = feature_rows(theta_x, theta_z, 236, 2.0, 0.4, 6)
    assert np.array_equal(xg[:, 4:], fg[:, 4:].astype(np.float32)) and np.array_equal(xj[:, 2:], fj[:, 2:].astype(np.float32))
    assert not xg[:, 2].any() and not xg[:, 10].any() and not xj[:, 6:].any()
    rowptr, col = pc.table_of(v["gj"][::-1], 118)
    r = pc.restate(rowptr, col, xj)
    # (ggnn_grain_centres sums a row in an order of its own: up to n - 1 roundings of a sum of n values below 2, twice)
    assert np.abs(xg[:, :2] - r["centre"]).max() <= 2 * int(r["sides"].max()) * 2 * U32
    # edge lengths: the minimum-image distance of the two ends, fp32
    for et in EDGE_TYPES:
        src, dst = EI[et].cpu().numpy()
        d = X[et[0]].cpu().numpy()[src, :2].astype(np.float64) - X[et[2]].cpu().numpy()[dst, :2]
        d -= np.rint(d)
        got = EA[et].cpu().numpy()
        assert got.shape == (708, 1) and got.dtype == np.float32
        assert np.abs(got[:, 0] - np.hypot(d[:, 0], d[:, 1])).max() <= 8 * U32, et
    # every grain's centre lies within a pixel or two of the reference's for the same grain (same ids: the image is its own)
    assert periodic_gap(xg[:, :2], g40["x_grain"][:, :2]).max() < 0.02

    R, Cm = product_models(10020, 1.0, DEV)
    ro = GrainRollout(R, Cm, X, EI, EA, 6, refresh_centres=True)
    ro.enable_events({"grain": np.ones((118, 1)), "joint": np.ones((236, 1))}, 1e-4, 0.6)
    ro.enable_polygons(capacity=2)
    for _ in range(2):
        pred = ro.step_events()[0]
        assert all(bool(torch.isfinite(t).all()) for t in pred.values())
    assert not ro.range_exceeded() and ro.polygons()["layers"] == 2
    ro.state()
    layer0 = ro.grain_image((501, 501), layer=0)
    share, want = cached(("round trip", "init"), lambda: round_trip(v, image, 118))
    assert np.array_equal(layer0.cpu().numpy(), want)
    error = ro.image_error(layer0, dev_image)
    assert error["differing"] == int((want != image).sum()) and error["rate"] == share
