"""Linking junctions by tracing boundaries (ggnn_image_junction_windows_traj / ggnn_junction_links_trace_traj, vectorize's
links="trace") against the restatement of tests/tracecheck.py.

What the rule is for.  Two grains that share two separate stretches of boundary -- a lens on a boundary one frame before it
vanishes, a band from wall to wall -- leave four junctions that hold the same pair, so the rule "the one other junction that
holds both grains" leaves those columns open and the image invalid, though it is a legal structure.  Following the boundary in
the image says which two junctions each stretch joins.  The CPU tests pin the restatement on the two measured cases (frame 36 of
the recorded phase-field sequence; a band between two walls), on every image the vectorise tests call valid (nothing changes
there), on a raster that Euler's formula rules out (nothing is repaired there) and on hand-made images for every way a walk
ends.  The GPU tests hold the kernels to the restatement bit for bit: xy, triples, the edge lists, the status, rep and the
three counters.

The property test.  32 x 32 periodic Voronoi images of 3 x 3 jittered seeds (trackcheck.moving_seeds, seeds 0, 3 and 6: the
ones of 0 .. 7 whose longest straight vertical stretch of boundary has at least 10 rows, found by looking at the images, not at
the rule's output) with a lens of 2 .. 12 pixels carrying a new id on that stretch: a strip one pixel wide beside the boundary
(k = 2 .. 7 pixels) or two wide across it (8, 10, 12).  The lens's two junctions are k rows apart (k / 2 for the wide ones), and
the junction rule merges windows within merge_radius into ONE junction, which Euler's formula then rules out whatever the
linking: so a lens is drawn with merge_radius = 1 when its junctions are two rows apart and with the default 2 otherwise, and
the images are valid at both radii before the lens."""
import ctypes
import os

import numpy as np
import pytest
import torch

import test_vectorize as tv
import test_vectorize_noflux as tn
import test_vectorize_union as tu
import tracecheck as tc
import trackcheck as tk
import vectorcheck as vc
import vectorcheck_noflux as vn
import vectorcheck_union as vu
from helpers import GOLDEN, ROOT, assert_close, oracle_models, product_models
from graingraphnn_amd import _lib
from graingraphnn_amd import vectorize as vz
from graingraphnn_amd.synthetic import EDGE_TYPES

DEV = "cuda"
GJ, JG, JJ = EDGE_TYPES
W = 7
C = len(tc.COUNTERS)
NO_TRACE = dict.fromkeys(tc.COUNTERS, 0)

cached = tv.cached


def traced(key, image, n_grain, boundary="periodic", **kw):
    """The restatement of a named image with its open pairs traced, computed once and left unchanged."""
    return cached(("traced", key, boundary, tuple(sorted(kw.items()))), lambda: tc.vectorize(image, n_grain, boundary=boundary, **kw))


def traced_union(key, images, n_grains, boundary, **kw):
    return cached(("traced union", key, boundary, tuple(sorted(kw.items()))),
                  lambda: tc.vectorize_union(images, n_grains, boundary=boundary, **kw))


def partners(v, j):
    return v["jj"][1, 3 * j:3 * j + 3].tolist()


def assert_symmetric(v, before):
    """Every traced column has its reverse: partner(partner(j)) == j for the same pair of grains."""
    n_traced = 0
    for s in np.nonzero((before == -1) & (v["jj"][1] >= 0))[0]:
        j, k = divmod(int(s), 3)
        o = int(v["jj"][1, s])
        pair = {int(v["triples"][j, a]) for a in tc.PAIRS[k]}
        back = [c for c, (a, b) in enumerate(tc.PAIRS) if {int(v["triples"][o, a]), int(v["triples"][o, b])} == pair]
        assert len(back) == 1 and before[3 * o + back[0]] == -1 and v["jj"][1, 3 * o + back[0]] == j, (j, k, o)
        n_traced += 1
    return n_traced


# ---- the images --------------------------------------------------------------------------------------------------------------

def frames():
    """The recorded sequence 0, 6, .., 48: pf_frames_cfg1.npz and its tail."""
    def make():
        head, tail = np.load(os.path.join(GOLDEN, "pf_frames_cfg1.npz")), np.load(os.path.join(GOLDEN, "pf_frames_cfg1_tail.npz"))
        d = {k: head[k] for k in ("theta_x", "theta_z", "G", "R")}
        for k in ("frames", "frame_ids", "extra_volume", "event_frame", "event_grain"):
            d[k] = np.concatenate([head[k], tail[k]])
        return d
    return cached("nine frames", make)


def band_image(ny=24, nx=32):
    """A band from wall to wall: the pair (outside, band) is held by two junctions on the left wall and two on the right."""
    img = np.zeros((ny, nx), np.int32)
    img[0:8, 0:nx // 2], img[0:8, nx // 2:] = 2, 3
    img[8:16, :] = 4
    img[16:, 0:10], img[16:, 10:22], img[16:, 22:] = 5, 6, 7
    return img, 7


def band_and_wall_lens():
    """24 x 40, no-flux: the band, and grain 8 as a lens on the top wall inside grain 2 -- the pair (outside, 2) twice there."""
    img, _ = band_image(24, 40)
    img[0:3, 4:8] = 8
    return img, 8


def halves(lens=True):
    """16 x 16, no-flux: two grains side by side -- the sphere of three faces, valid --, and grain 4 as a lens on their boundary,
    a strip of five pixels beside it."""
    img = np.full((16, 16), 2, np.int32)
    img[:, 8:] = 3
    if lens:
        img[5:10, 7] = 4
    return img


def lens_image(checkerboard=False):
    """32 x 32, periodic: test_vectorize's plain bricks with grain 17 as a lens of three pixels on the boundary of bricks 1 and 2;
    checkerboard: the two pixels of row 1 beside that boundary exchanged, [1 2; 2 1] on the way from the lens up to the bricks'
    junction."""
    plain, n = tv.case("plain")[:2]
    img = plain.copy()
    img[4:7, 7] = n + 1
    if checkerboard:
        img[1, 7], img[1, 8] = plain[1, 8], plain[1, 7]
    return img, n + 1


def single_pixel_image():
    """32 x 32, periodic: the plain bricks with grain 17 as ONE pixel beside the 1 | 2 boundary: its two windows merge into one
    junction, which the 1 | 2 boundary leaves twice.  33 junctions: an odd count for the unions below."""
    plain, n = tv.case("plain")[:2]
    img = plain.copy()
    img[4, 7] = n + 1
    return img, n + 1


def straight_stretch(img):
    """The longest vertical stretch of boundary: (x, y0, rows) with img[y, x - 1] = a != b = img[y, x] for y0 <= y < y0 + rows."""
    best = (0, 0, 0)
    for x in range(1, img.shape[1]):
        y = 0
        while y < img.shape[0]:
            a, b, y1 = img[y, x - 1], img[y, x], y
            while a != b and y1 + 1 < img.shape[0] and img[y1 + 1, x - 1] == a and img[y1 + 1, x] == b:
                y1 += 1
            if a != b and y1 - y + 1 > best[2]:
                best = (x, y, y1 - y + 1)
            y = y1 + 1
    return best


LENS_PIXELS = (2, 3, 4, 5, 6, 7, 8, 10, 12)
LENS_SEEDS = (0, 3, 6)


def voronoi_with_lens(seed, pixels):
    """-> (the Voronoi image, the same with the lens, the merge radius the lens is drawn for)."""
    base = tk.voronoi(tk.moving_seeds(32, 32, 3, 1, seed)[0], 32, 32)
    x, y0, rows = straight_stretch(base)
    wide = pixels >= 8
    k = pixels // 2 if wide else pixels
    assert rows >= k + 2
    top = y0 + (rows - k) // 2
    img = base.copy()
    img[top:top + k, x - 1] = 10
    if wide:
        img[top:top + k, x] = 10
    return base, img, 1 if k == 2 else 2


# ---- CPU: the restatement ----------------------------------------------------------------------------------------------------

def test_frame_36_of_the_recorded_sequence():
    """Grain 26 (1-based) is a lens on the boundary of grains 86 and 95 one frame before the reference eliminates it."""
    d = frames()
    assert d["frame_ids"].tolist() == list(range(0, 49, 6)) and (37, 26) in zip(d["event_frame"].tolist(), d["event_grain"].tolist())
    image = d["frames"][6].astype(np.int32)
    assert int((image == 26).sum()) == 33
    before = tv.restated("frame 36", image, 118, "points")
    v = traced("frame 36", image, 118, grid="points")
    assert before["status"]["n_open_pairs"] == 4 and before["status"]["n_joint"] == 200 and not vc.is_valid(before["status"])
    assert before["status"]["n_present_grains"] == 100
    assert v["n_open_before"] == 4 and v["status"]["n_open_pairs"] == 0 and vc.is_valid(v["status"])
    assert v["counters"] == dict(n_traced=4, n_trace_failed=0, n_trace_overflow=0)
    assert [tuple(v["triples"][j]) for j in (93, 97, 101, 105)] == [(85, 94, 95), (25, 85, 94), (25, 85, 94), (51, 85, 94)]
    assert partners(v, 93)[0] == 97 and partners(v, 97)[2] == 93 and partners(v, 101)[2] == 105 and partners(v, 105)[2] == 101
    changed = np.nonzero(before["jj"][1] != v["jj"][1])[0].tolist()
    assert changed == [3 * 93, 3 * 97 + 2, 3 * 101 + 2, 3 * 105 + 2] and assert_symmetric(v, before["jj"][1]) == 4
    for k in ("xy", "triples", "gj"):
        assert np.array_equal(before[k], v[k]), k


def test_a_band_from_wall_to_wall():
    image, n_grain = band_image()
    for grid in ("cells", "points"):
        before = tn.restated("band", image, n_grain, grid)
        s = before["status"]
        assert s["n_joint"] == 10 == 2 * s["n_present_grains"] - 2 and s["n_open_pairs"] == 4 and not vn.is_valid(s)
        assert [j for j in range(10) if -1 in partners(before, j)] == [1, 3, 4, 7]
        assert all({0, 3} <= set(before["triples"][j].tolist()) for j in (1, 3, 4, 7))      # the pair (outside, band), four times
        v = traced("band", image, n_grain, "noflux", grid=grid)
        assert vn.is_valid(v["status"]) and v["counters"] == dict(n_traced=4, n_trace_failed=0, n_trace_overflow=0)
        assert partners(v, 1)[1] == 4 and partners(v, 4)[0] == 1 and partners(v, 3)[1] == 7 and partners(v, 7)[0] == 3
        assert assert_symmetric(v, before["jj"][1]) == 4


def valid_images():
    """name -> (image, n_grain, boundary, keywords): what the vectorise tests call valid."""
    out = {}
    for tag in ("init", "step1", "step3", "mass3"):
        out["phase field " + tag] = (tv.pde_image(tag), 118, "periodic", dict(grid="points"))
    for size in (96, 128, 256):
        out[f"graph_40 at {size}"] = (tv.fixture_raster("graph_40", size), 118, "periodic", {})
    out["graph_120 at 1024"] = (tv.fixture_raster("graph_120", 1024), 1043, "periodic", {})
    out["generated_80 at 512"] = (tv.fixture_raster("generated_80_seed7", 512), npz_grains("generated_80_seed7"), "periodic", {})
    for name in tv.CASE_NAMES:
        image, n, kw, want = tv.case(name)
        if want.get("valid"):
            out["bricks: " + name] = (image, n, "periodic", kw)
    for size in (256, 128):
        for grid in ("cells", "points"):
            out[f"noflux_40 at {size}, {grid}"] = (tn.fixture_raster("noflux_40_seed1", size), 101, "noflux", dict(grid=grid))
    for ny, nx in ((32, 32), (24, 40)):
        out[f"walls {ny} x {nx}"] = (tn.walls_image(ny, nx)[0], 7, "noflux", {})
        for b in tu.BOUNDARIES:
            for i, (image, n) in enumerate(zip(*tu.stack_of(b, ny, nx))):
                out[f"stack {b} {ny} x {nx} [{i}]"] = (image, n, b, {})
    for name in tn.VARIANTS:
        image, n, kw, want, _ = tn.variant(name)
        if want.get("valid"):
            out["walls: " + name] = (image, n, "noflux", kw)
    for nx in (255, 256, 257):
        out[f"strip {nx}"] = (tn.strip(nx) + ("noflux", {}))
    return out


def test_a_structure_without_open_pairs_comes_out_as_it_was():
    cases = valid_images()
    assert len(cases) >= 30
    n_valid = 0
    for name, (image, n_grain, boundary, kw) in cases.items():
        one = vc.vectorize if boundary == "periodic" else vn.vectorize
        before = one(image, n_grain, **kw)
        if not tc.is_valid(before["status"], boundary):
            assert name.startswith("stack periodic"), name      # (the walls image read as a torus is no valid structure)
            continue
        n_valid += 1
        v = tc.vectorize(image, n_grain, boundary=boundary, **kw)
        assert v["counters"] == NO_TRACE and v["n_open_before"] == 0 and v["status"] == before["status"], name
        for k in ("xy", "triples", "gj", "jj"):
            assert v[k].dtype == before[k].dtype and np.array_equal(v[k], before[k]), (name, k)
        W_ = tc.Windows(image, n_grain, kw.get("merge_radius", 2), boundary)
        assert len(v["rep"]) == len(v["triples"]) and v["rep"].dtype == np.int32
        assert all(tuple(v["triples"][j]) in W_.keys(*W_.window(v["rep"][j])) for j in range(len(v["rep"]))), name
    assert n_valid >= 30


def npz_grains(name):
    return tv.npz(name)["x_grain"].shape[0]


def test_a_structure_that_fails_eulers_formula_is_not_repaired():
    """generated_40_seed1 at 256: sub-pixel edges lost a junction; the pairs left open have no boundary to follow."""
    image = tv.fixture_raster("generated_40_seed1", 256)
    before = tv.restated(("generated_40_seed1", 256), image, 115)
    v = traced(("generated_40_seed1", 256), image, 115)
    s = v["status"]
    assert not vc.is_valid(s) and s["n_joint"] != 2 * s["n_present_grains"]
    assert s["n_open_pairs"] == before["status"]["n_open_pairs"] - v["counters"]["n_traced"]
    assert int((v["jj"][1] == -1).sum()) == s["n_open_pairs"] == v["counters"]["n_trace_failed"] + v["counters"]["n_trace_overflow"]
    assert assert_symmetric(v, before["jj"][1]) == v["counters"]["n_traced"]
    closed = before["jj"][1] != -1
    assert np.array_equal(v["jj"][1][closed], before["jj"][1][closed])          # what was linked stays as it was


def test_hand_made_a_lens_between_two_walls_and_max_trace():
    """The walks of `halves`: five vertices from the top wall's junction down to the lens, six from the lens down to the bottom
    wall's.  max_trace one below the length of a walk overflows, both ways; at the length it links."""
    assert vn.is_valid(vn.vectorize(halves(False), 3)["status"])
    before = vn.vectorize(halves(), 4)
    assert before["status"]["n_joint"] == 4 and before["status"]["n_open_pairs"] == 4
    assert [tuple(t) for t in before["triples"].tolist()] == [(0, 1, 2), (1, 2, 3), (1, 2, 3), (0, 1, 2)]
    Wn = tc.Windows(halves(), 4, 2, "noflux")
    v = traced("halves", halves(), 4, "noflux")
    T = tc.Tracer(Wn, v["triples"], v["rep"])
    assert [T.partner(j, 1, 2, 100) for j in range(4)] == [("n_traced", 1, 5), ("n_traced", 0, 5), ("n_traced", 3, 6), ("n_traced", 2, 6)]
    assert vn.is_valid(v["status"]) and v["jj"][1].tolist() == [3, 3, 1, 0, 2, 2, 3, 1, 1, 0, 0, 2]
    for limit, (n_traced, n_over), jj in ((4, (0, 4), [3, 3, -1, -1, 2, 2, -1, 1, 1, 0, 0, -1]),
                                          (5, (2, 2), [3, 3, 1, 0, 2, 2, -1, 1, 1, 0, 0, -1]),
                                          (6, (4, 0), [3, 3, 1, 0, 2, 2, 3, 1, 1, 0, 0, 2])):
        v = traced("halves", halves(), 4, "noflux", max_trace=limit)
        assert v["counters"] == dict(n_traced=n_traced, n_trace_failed=0, n_trace_overflow=n_over), limit
        assert v["jj"][1].tolist() == jj and v["status"]["n_open_pairs"] == n_over
    assert tc.default_max_trace(16, 16) == 128


def checkerboard_halves():
    img = halves()
    img[2, 7], img[2, 8] = 3, 2
    return img


def staircase_halves():
    img = halves()
    img[10, 8] = 4
    return img


def single_pixel_halves():
    img = halves(False)
    img[7, 7] = 4
    return img


def four_quadruples():
    """16 x 16, periodic: four bricks that meet in four quadruple windows: every triple twice, every pair four times, all 24
    columns open; the two junctions of a quadruple window are each other's partner for its (TL, BR)."""
    return tv.bricks(16, 16, [0, 8], [[0, 8], [0, 8]])


def test_hand_made_the_ways_a_walk_ends():
    # a checkerboard window [2 3; 3 2] between the top wall and the lens: both walks through it fail, the other two link
    v = traced("checkerboard", checkerboard_halves(), 4, "noflux")
    assert tc.Windows(checkerboard_halves(), 4, 2, "noflux").pixels(1, 7) == (2, 3, 3, 2)
    assert v["counters"] == dict(n_traced=2, n_trace_failed=2, n_trace_overflow=0) and v["status"]["n_open_pairs"] == 2
    assert v["jj"][1].tolist() == [3, 3, -1, -1, 2, 2, 3, 1, 1, 0, 0, 2] and not vn.is_valid(v["status"])
    # a staircase of two pixels under the lens: its lower junction has two carriers, (9, 7) the representative and (10, 7),
    # and the 2 | 3 boundary leaves it from (10, 7) alone
    img = staircase_halves()
    v = traced("staircase", img, 4, "noflux")
    Wn = tc.Windows(img, 4, 2, "noflux")
    T = tc.Tracer(Wn, v["triples"], v["rep"])
    assert v["status"]["n_merged_windows"] == 1 and Wn.window(v["rep"][2]) == (9, 7) and T.owned(2, 10, 7) and T.owned(2, 9, 7)
    assert T.exits(2, 1, 2) == ([(11, 7, 1)], []) and not any(set(c) == {2, 3} for c in Wn.cracks(9, 7))
    assert v["counters"] == dict(n_traced=4, n_trace_failed=0, n_trace_overflow=0) and vn.is_valid(v["status"])
    assert v["jj"][1].tolist() == [3, 3, 1, 0, 2, 2, 3, 1, 1, 0, 0, 2]
    # a lens of ONE pixel: its two windows are one junction, which the 2 | 3 boundary leaves twice: open on both sides, and at
    # the walls' junctions, whose walks arrive there
    img = single_pixel_halves()
    v = traced("single pixel", img, 4, "noflux")
    T = tc.Tracer(tc.Windows(img, 4, 2, "noflux"), v["triples"], v["rep"])
    assert [tuple(t) for t in v["triples"].tolist()] == [(0, 1, 2), (1, 2, 3), (0, 1, 2)] and len(T.exits(1, 1, 2)[0]) == 2
    assert v["counters"] == dict(n_traced=0, n_trace_failed=5, n_trace_overflow=0)
    assert v["jj"][1].tolist() == [2, 2, -1, -1, -1, -1, 0, 0, -1]
    # four quadruple windows on a torus of four grains
    img, n = four_quadruples()
    before = vc.vectorize(img, n)
    assert before["status"]["n_quad_windows"] == 4 and before["status"]["n_open_pairs"] == 24 and (before["jj"][1] == -1).all()
    v = traced("four quadruples", img, n)
    assert v["counters"] == dict(n_traced=24, n_trace_failed=0, n_trace_overflow=0) and vc.is_valid(v["status"])
    assert assert_symmetric(v, before["jj"][1]) == 24
    Wp = tc.Windows(img, n, 2, "periodic")
    T = tc.Tracer(Wp, v["triples"], v["rep"])
    assert [Wp.window(r) for r in v["rep"]] == [(7, 7), (7, 7), (7, 15), (7, 15), (15, 7), (15, 7), (15, 15), (15, 15)]
    n_diagonal = 0
    for j in range(8):
        for k, (a, b) in enumerate(tc.PAIRS):
            found, diagonals = T.exits(j, int(v["triples"][j, a]), int(v["triples"][j, b]))
            if diagonals:
                n_diagonal += 1
                assert diagonals == [Wp.window(v["rep"][j])] and v["jj"][1, 3 * j + k] == j ^ 1, (j, k)
            else:
                assert len(found) == 1 and T.partner(j, int(v["triples"][j, a]), int(v["triples"][j, b]), 64)[2] == 8
    assert n_diagonal == 8


@pytest.mark.parametrize("seed", LENS_SEEDS)
def test_property_a_lens_on_a_voronoi_boundary(seed):
    for pixels in LENS_PIXELS:
        base, img, R = voronoi_with_lens(seed, pixels)
        assert int((img == 10).sum()) == pixels and base.max() == 9
        for radius in (1, 2):
            assert vc.is_valid(vc.vectorize(base, 9, merge_radius=radius)["status"]), (seed, radius)
        before = vc.vectorize(img, 10, merge_radius=R)
        assert before["status"]["n_open_pairs"] == 4 and not vc.is_valid(before["status"]), (seed, pixels)
        v = tc.vectorize(img, 10, merge_radius=R)
        assert vc.is_valid(v["status"]) and v["counters"] == dict(n_traced=4, n_trace_failed=0, n_trace_overflow=0), (seed, pixels)
        assert assert_symmetric(v, before["jj"][1]) == 4


def test_restatement_of_a_union():
    """Valid, lens, failing: per-image statuses and counters; every image's rows are its own call's."""
    images, n_grains = union_stack("periodic")
    u = traced_union("three", images, n_grains, "periodic")
    assert u["counters"] == [NO_TRACE, dict(n_traced=4, n_trace_failed=0, n_trace_overflow=0),
                             dict(n_traced=2, n_trace_failed=2, n_trace_overflow=0)]
    assert [s["n_open_pairs"] for s in u["status"]] == [0, 0, 2] and u["joint_off"] == [0, 32, 66, 100]
    for b, (image, n) in enumerate(zip(images, n_grains)):
        v = tc.vectorize(image, n)
        j0, j1 = u["joint_off"][b], u["joint_off"][b + 1]
        own = u["jj"][1, 3 * j0:3 * j1]
        assert np.array_equal(np.where(own >= 0, own - j0, own), v["jj"][1]) and np.array_equal(u["rep"][j0:j1], v["rep"])
        assert u["status"][b] == v["status"] and u["counters"][b] == v["counters"]


def union_stack(boundary):
    if boundary == "periodic":
        made = [tv.case("plain")[:2], lens_image(), lens_image(True)]
    else:
        made = [(tn.walls_image(24, 40)[0], 7), band_and_wall_lens(), band_with_a_pixel_on_the_wall()]
    return [np.ascontiguousarray(m[0]) for m in made], [m[1] for m in made]


def band_with_a_pixel_on_the_wall():
    """The 24 x 40 band with grain 8 as ONE pixel on the left wall inside it: its two windows are one junction, which the
    boundary (outside | band) leaves twice, so the walks along the left wall are refused there; the right wall's link."""
    img, _ = band_image(24, 40)
    img[11, 0] = 8
    return img, 8


def test_entry_points_validate_on_the_host():
    lib = _lib.load()
    assert lib.ggnn_version() == 26 == _lib.GGNN_ABI_VERSION
    assert {"ggnn_image_junction_windows_traj", "ggnn_junction_links_trace_traj"} <= set(_lib.EXPORTED_SYMBOLS)
    assert lib.ggnn_image_junction_windows_traj(None, None, None) == -1 and lib.ggnn_junction_links_trace_traj(None, None) == -1
    buf = (ctypes.c_int64 * 64)()                 # (host memory: refused before anything would be launched)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def windows(rep, **kw):
        A = _lib.JunctionTrajArgs(p, p, p, p, p, p, p, p, 4 * 3 * 32, 32, 32, 3, 16, 8, 1.0, 1.0 / 32, 2, 0)
        A.images = None                           # (so that a call that passes every other check still launches nothing)
        for k, v in kw.items():
            setattr(A, k, v)
        return lib.ggnn_image_junction_windows_traj(ctypes.byref(A), rep, None)
    assert windows(p) == -1 and windows(None, images=p) == -1
    for bad in (dict(grain_off=None), dict(status=p.value + 4), dict(merge_radius=8), dict(nx=4), dict(n_grain=0),
                dict(joint_capacity=0), dict(pitch=0.0), dict(boundary=2), dict(n_image=0), dict(workspace_bytes=4 * 96 - 1)):
        assert windows(p, images=p, **bad) == -1, bad

    def trace(**kw):
        A = _lib.LinkTraceArgs(p, p, p, p, p, p, p, p, p, 32, 32, 3, 16, 8, 24, 128, 2, 0)
        A.images = None
        for k, v in kw.items():
            setattr(A, k, v)
        return lib.ggnn_junction_links_trace_traj(ctypes.byref(A), None)
    assert trace() == -1
    for bad in (dict(grain_off=None), dict(triples=None), dict(rep=None), dict(rowptr=None), dict(col=None), dict(edge_jj=None),
                dict(status=None), dict(counters=None), dict(status=p.value + 4), dict(edge_jj=p.value + 4),
                dict(counters=p.value + 4), dict(grain_off=p.value + 4), dict(rep=p.value + 2), dict(triples=p.value + 1),
                dict(n_grain=0), dict(n_grain=2 ** 31 - 2), dict(joint_capacity=0), dict(joint_capacity=2 ** 31 // 3 + 1),
                dict(E_cap=-1), dict(E_cap=2 ** 31 - 1), dict(n_image=0), dict(n_image=_lib.GGNN_JUNCTION_MAX_BLOCKS + 1),
                dict(merge_radius=-1), dict(merge_radius=8), dict(nx=4), dict(ny=4), dict(nx=1 << 15), dict(ny=1 << 15),
                dict(boundary=2), dict(boundary=-1), dict(max_trace=0), dict(max_trace=-5)):
        assert trace(images=p, **bad) == -1, bad


def test_header_binding_and_struct_sizes_agree():
    import re
    src = open(os.path.join(ROOT, "include", "ggnn.h")).read()
    assert re.search(r"#define GGNN_ABI_VERSION 26\b", src) and f"#define GGNN_TRACE_COUNTERS {_lib.GGNN_TRACE_COUNTERS}" in src
    body = re.search(r"typedef struct ggnn_link_trace_args \{(.*?)\} ggnn_link_trace_args;", src, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in _lib.LinkTraceArgs._fields_]
    assert ctypes.sizeof(_lib.LinkTraceArgs) == 9 * 8 + 7 * 8 + 2 * 4
    assert ctypes.sizeof(_lib.JunctionTrajArgs) == 9 * 8 + 5 * 8 + 4 * 4 and ctypes.sizeof(_lib.LinkTrajArgs) == 5 * 8 + 4 * 8
    assert vz.TRACE_COUNTERS == tc.COUNTERS and _lib.GGNN_TRACE_COUNTERS == C


def test_python_entry_points_refuse_another_links_value():
    host = torch.ones(2, 8, 8, dtype=torch.int32)
    z = np.zeros(2)
    for call in (lambda **kw: vz.graph_from_image(host[0], 1, **kw), lambda **kw: vz.graphs_from_images(host, [1, 1], **kw),
                 lambda **kw: vz.sample_from_image(host[0], z, z, 2.0, 0.4, span=6, **kw),
                 lambda **kw: vz.samples_from_images(host, [z, z], [z, z], 2.0, 0.4, span=6, **kw),
                 lambda **kw: vz.frames_to_samples(host, z, z, 2.0, 0.4, span=6, **kw),
                 lambda **kw: vz.track_frames(host, 2, **kw)):
        with pytest.raises(ValueError, match="links must be 'unique' or 'trace'"):
            call(links="walk")
        with pytest.raises(ValueError, match="max_trace must be at least 1"):
            call(links="trace", max_trace=0)
        with pytest.raises(_lib.GGNNError, match="device tensor"):   # (a host image gets as far as it did)
            call(links="trace")


# ---- GPU: the kernels equal the restatement bit for bit ------------------------------------------------------------------------

def to_dev(images):
    return torch.from_numpy(np.stack(images).astype(np.int32)).to(DEV)


def statuses(v):
    """The restatement's status dicts as links="trace" returns them: with the three counters."""
    if isinstance(v["status"], dict):
        return dict(v["status"], **v["counters"])
    return [dict(s, **c) for s, c in zip(v["status"], v["counters"])]


def assert_single_equals(got, v, what):
    """graph_from_image(links="trace")'s result against tracecheck.vectorize's."""
    xy, triples, ei, status = got[:4]
    assert status == statuses(v), (what, status, statuses(v))
    assert np.array_equal(xy.cpu().numpy().view(np.uint32), v["xy"].view(np.uint32)) and xy.dtype == torch.float32, what
    assert np.array_equal(triples.cpu().numpy(), v["triples"]) and triples.dtype == torch.int32, what
    assert np.array_equal(ei[GJ].cpu().numpy(), v["gj"]) and np.array_equal(ei[JG].cpu().numpy(), v["gj"][::-1]), what
    assert np.array_equal(ei[JJ].cpu().numpy(), v["jj"]) and all(ei[et].dtype == torch.int64 and ei[et].is_contiguous() for et in EDGE_TYPES), what
    if len(got) > 4:
        assert got[4] == v["corner_grains"] and got[5] == float(v["max_y"]), what


def assert_union_equals(res, held, u, what):
    """graphs_from_images(links="trace")'s result and the arrays behind it against tracecheck.vectorize_union's."""
    n = len(u["xy"])
    assert res["status"] == statuses(u), (what, res["status"], statuses(u))
    assert res["traj_offsets"]["grain"] == u["grain_off"] and res["traj_offsets"]["joint"] == [min(o, n) for o in u["joint_off"]]
    assert np.array_equal(res["xy"].cpu().numpy().view(np.uint32), u["xy"].view(np.uint32)), what
    assert np.array_equal(res["triples"].cpu().numpy(), u["triples"]), what
    ei = res["edge_index_dict"]
    assert np.array_equal(ei[GJ].cpu().numpy(), u["gj"]) and np.array_equal(ei[JG].cpu().numpy(), u["gj"][::-1]), what
    assert np.array_equal(ei[JJ].cpu().numpy(), u["jj"]), what
    assert held["rep"].dtype == torch.int32 and np.array_equal(held["rep"][:n].cpu().numpy(), u["rep"]), what
    assert not held["rep"][n:].any()
    if "corner_grains" in u:
        assert res["corner_grains"] == u["corner_grains"] and res["max_y"] == float(u["max_y"]), what


def run_union(images, n_grains, boundary, **kw):
    return vz._graphs(to_dev(images), n_grains, kw.pop("grid", "cells"), kw.pop("merge_radius", 2), kw.pop("joint_capacity", None), False,
                      boundary, "trace", kw.pop("max_trace", None))


SMALL = {"lens 32 x 32": lambda: lens_image() + ("periodic",), "band 24 x 32": lambda: band_image() + ("noflux",),
         "band and a lens on a wall 24 x 40": lambda: band_and_wall_lens() + ("noflux",),
         "checkerboard": lambda: (checkerboard_halves(), 4, "noflux"), "staircase": lambda: (staircase_halves(), 4, "noflux"),
         "single pixel": lambda: (single_pixel_halves(), 4, "noflux"), "four quadruples": lambda: four_quadruples() + ("periodic",),
         "lens with a checkerboard": lambda: lens_image(True) + ("periodic",),
         # the same walks along rows: a walk turns with the image, and UP | DOWN and LEFT | RIGHT are separate code
         "lens transposed": lambda: (np.ascontiguousarray(lens_image()[0].T), 17, "periodic"),
         "halves transposed": lambda: (np.ascontiguousarray(halves().T), 4, "noflux")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SMALL))
def test_kernels_on_small_shapes(name):
    image, n_grain, boundary = SMALL[name]()
    dev = torch.from_numpy(image).to(DEV)
    for grid in ("cells", "points"):
        v = traced(name, image, n_grain, boundary, grid=grid)
        got = vz.graph_from_image(dev, n_grain, grid=grid, strict=False, boundary=boundary, links="trace")
        assert_single_equals(got, v, (name, grid))
        res, held = run_union([image], [n_grain], boundary, grid=grid)
        assert_union_equals(res, held, traced_union(name, [image], [n_grain], boundary, grid=grid), (name, grid))
        if tc.is_valid(v["status"], boundary):
            assert_single_equals(vz.graph_from_image(dev, n_grain, grid=grid, boundary=boundary, links="trace"), v, name)
        else:
            with pytest.raises(ValueError, match="n_open_pairs"):
                vz.graph_from_image(dev, n_grain, grid=grid, boundary=boundary, links="trace")
    if name == "band and a lens on a wall 24 x 40":
        assert v["counters"]["n_traced"] == 8 and vn.is_valid(v["status"])
    if name == "lens 32 x 32":
        assert v["counters"]["n_traced"] == 4 and vc.is_valid(v["status"])
        for limit in (3, 4):                     # the walks of this image reach four vertices above the lens and one below it
            w = traced(name, image, n_grain, boundary, max_trace=limit)
            assert w["counters"]["n_trace_overflow"] == (2 if limit == 3 else 0) and w["counters"]["n_traced"] == limit + limit - 4
            assert_single_equals(vz.graph_from_image(dev, n_grain, strict=False, links="trace", max_trace=limit), w, limit)


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", tu.BOUNDARIES)
def test_a_union_of_a_valid_a_traced_and_a_failing_image(boundary):
    images, n_grains = union_stack(boundary)
    u = traced_union("three", images, n_grains, boundary)
    assert [c["n_traced"] > 0 for c in u["counters"]] == [False, True, True] and u["counters"][2]["n_trace_failed"] > 0
    assert [tc.is_valid(s, boundary) for s in u["status"]] == [True, True, False]
    res, held = run_union(images, n_grains, boundary)
    assert_union_equals(res, held, u, boundary)
    dev = to_dev(images)
    for t in range(3):
        own = vz.graph_from_image(dev[t], n_grains[t], strict=False, boundary=boundary, links="trace")
        tu.assert_same_graph(vz.union_member(res, t), own, (boundary, t))
    with pytest.raises(ValueError, match=rf"1 of 3 images are not valid {boundary}.*image 2: \{{.*'n_trace_failed': [1-9]"):
        vz.graphs_from_images(dev, n_grains, boundary=boundary, links="trace")
    # links="unique" on the same stack: the restatement of the parent's rule, and nothing more in the status
    plain = vz.graphs_from_images(dev, n_grains, strict=False, boundary=boundary)
    tu.assert_equals_restatement(plain, vu.vectorize(images, n_grains, boundary=boundary), boundary)
    assert all(set(s) == set(vz.STATUS_WORDS) for s in plain["status"])


def block_stack(total):
    """A periodic 32 x 32 union of `total` junctions whose traced lens image lies across column 256 of the joint->joint list,
    the edge of the first block of threads: -> (images, n_grains)."""
    plain, lens, single, nine = tv.case("plain")[:2], lens_image(), single_pixel_image(), tu.nine_bricks(32, 32)
    counts = {id(plain): 32, id(lens): 34, id(single): 33, id(nine): 18}
    front = [plain, nine, nine]                                 # 68 junctions, then the lens: columns 204 .. 305
    tail = {153: [single] * 3 + [nine] * 3, 154: [plain] * 2 + [nine] * 5, 155: [single, plain] + [nine] * 5}[total - 68 - 34]
    made = front + [lens] + tail
    assert sum(counts[id(m)] for m in made) == total
    return [np.ascontiguousarray(m[0]) for m in made], [m[1] for m in made]


@pytest.mark.gpu
@pytest.mark.parametrize("total", [255, 256, 257])
def test_unions_around_a_block_of_threads(total):
    images, n_grains = block_stack(total)
    u = traced_union(("block", total), images, n_grains, "periodic")
    assert u["joint_off"][-1] == total and u["counters"][3]["n_traced"] == 4
    opened = np.nonzero(vu.vectorize(images, n_grains)["jj"][1] == -1)[0]
    assert opened.min() < 256 <= opened.max()                  # open columns in the first block of threads and in the second
    res, held = run_union(images, n_grains, "periodic")
    assert_union_equals(res, held, u, total)


def guarded_trace(images, n_grains, boundary, cap, max_trace=None):
    """Both new entry points on guarded arrays -> (xy, triples, gj, jj, status, counts, rep, counters), 16 guard words of -7
    behind each."""
    from graingraphnn_amd.backend import default_backend
    lib, be, dev = _lib.load(), default_backend(), to_dev(images)
    B, ny, nx = dev.shape
    noflux = boundary == "noflux"
    n_total = sum(n_grains)
    _, off = vz.grain_offsets(n_grains, DEV)
    wy, wx = (ny + 1, nx + 1) if noflux else (ny, nx)
    n_blocks = B * wy * ((wx + 255) // 256)
    xy = torch.full((2 * cap + 16,), -7.0, dtype=torch.float32, device=DEV)
    triples = torch.full((3 * cap + 16,), -7, dtype=torch.int32, device=DEV)
    rep = torch.full((cap + 16,), -7, dtype=torch.int32, device=DEV)
    gj = torch.full((6 * cap + 16,), -7, dtype=torch.int64, device=DEV)
    jj = torch.full((6 * cap + 16,), -7, dtype=torch.int64, device=DEV)
    status = torch.full((B * W + B + 1 + 16,), -7, dtype=torch.int64, device=DEV)
    counters = torch.full((C * B + 16,), -7, dtype=torch.int64, device=DEV)
    counts = torch.full((n_total + 16,), -7, dtype=torch.int64, device=DEV)
    ws = torch.full((n_blocks + 16,), -7, dtype=torch.int32, device=DEV)
    A = _lib.JunctionTrajArgs(dev.data_ptr(), off.data_ptr(), counts.data_ptr(), xy.data_ptr(), triples.data_ptr(), gj.data_ptr(),
                              status.data_ptr(), ws.data_ptr(), 4 * n_blocks, nx, ny, B, n_total, cap, 1.0,
                              float(np.float32(1) / np.float32(nx)), 2, vz.BOUNDARIES[boundary])
    _lib.check(lib.ggnn_image_junction_windows_traj(ctypes.byref(A), rep.data_ptr(), _lib.current_stream()), "windows")
    rows = gj[:6 * cap].view(2, 3 * cap)
    n = min(int(status[B * W + B]), cap)
    table = torch.stack([rows[1, :3 * n], rows[0, :3 * n]]).contiguous()          # joint -> grain, the junctions written
    csr = be.build_csr_batch([(table, cap, n_total)])[0]
    L = _lib.LinkTrajArgs(triples.data_ptr(), csr.rowptr.data_ptr(), csr.col.data_ptr(), jj.data_ptr(), status.data_ptr(),
                          n_total, cap, csr.col.numel(), B)
    _lib.check(lib.ggnn_junction_links_traj(ctypes.byref(L), _lib.current_stream()), "ggnn_junction_links_traj")
    T = _lib.LinkTraceArgs(dev.data_ptr(), off.data_ptr(), triples.data_ptr(), rep.data_ptr(), csr.rowptr.data_ptr(),
                           csr.col.data_ptr(), jj.data_ptr(), status.data_ptr(), counters.data_ptr(), nx, ny, B, n_total, cap,
                           csr.col.numel(), 4 * (nx + ny) if max_trace is None else max_trace, 2, vz.BOUNDARIES[boundary])
    _lib.check(lib.ggnn_junction_links_trace_traj(ctypes.byref(T), _lib.current_stream()), "ggnn_junction_links_trace_traj")
    return xy, triples, gj, jj, status, counts, rep, counters


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", tu.BOUNDARIES)
def test_the_capacity_ends_inside_the_image_that_holds_the_lens(boundary):
    """Guarded arrays; a capacity that cuts the traced image between its junctions (an owner that was cut off owns nothing),
    and one with room to spare."""
    images, n_grains = union_stack(boundary)
    full = traced_union("three", images, n_grains, boundary)
    B, n_total = 3, sum(n_grains)
    cut = (full["joint_off"][1] + full["joint_off"][2]) // 2 + 1
    for cap in (cut, full["joint_off"][3] + 5):
        u = traced_union("three", images, n_grains, boundary, joint_capacity=cap)
        xy, triples, gj, jj, status, counts, rep, counters = guarded_trace(images, n_grains, boundary, cap)
        n = min(cap, full["joint_off"][3])
        words = status.tolist()
        assert [dict(zip(vz.STATUS_WORDS, words[b * W:(b + 1) * W])) for b in range(B)] == u["status"], cap
        assert words[B * W:B * W + B + 1] == full["joint_off"] and words[B * W + B + 1:] == [-7] * 16
        got = counters.tolist()
        assert [dict(zip(tc.COUNTERS, got[C * b:C * b + C])) for b in range(B)] == u["counters"] and got[C * B:] == [-7] * 16
        assert np.array_equal(xy[:2 * n].cpu().numpy().view(np.uint32), u["xy"].reshape(-1).view(np.uint32))
        assert np.array_equal(triples[:3 * n].cpu().numpy(), u["triples"].reshape(-1))
        assert np.array_equal(rep[:n].cpu().numpy(), u["rep"]) and bool((rep[n:] == -7).all())
        assert bool((xy[2 * n:] == -7).all()) and bool((triples[3 * n:] == -7).all())
        for lists, want in ((gj, u["gj"]), (jj, u["jj"])):
            rows = lists[:6 * cap].view(2, 3 * cap)
            assert np.array_equal(rows[:, :3 * n].cpu().numpy(), want)
            assert bool((rows[:, 3 * n:] == -7).all()) and bool((lists[6 * cap:] == -7).all())
        assert np.array_equal(counts[:n_total].cpu().numpy(), u["counts"]) and bool((counts[n_total:] == -7).all())
    assert traced_union("three", images, n_grains, boundary, joint_capacity=cut)["status"][1]["overflow"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", tu.BOUNDARIES)
def test_captured_graph_gives_the_same_bits(boundary):
    """Vectorise + links + trace in one captured graph, replayed twice: a replay starts from its own zeroed status and counters
    and from edge lists its links call has written anew."""
    images, n_grains = union_stack(boundary)
    u = traced_union("three", images, n_grains, boundary)
    dev = vz._stack(to_dev(images))
    off = vz.grain_offsets(n_grains, DEV)
    eager = vz._vectorize_union(dev, n_grains, "cells", 2, None, boundary, grain_off=off, links="trace")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = vz._vectorize_union(dev, n_grains, "cells", 2, None, boundary, grain_off=off, links="trace")
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for k in ("xy", "triples", "gj", "jj", "status", "counts", "rep"):
        assert torch.equal(held[k], eager[k]), k
    res, _ = vz._graphs_of(held, held["status"].tolist(), False)
    assert_union_equals(res, held, u, boundary)


# links="unique", recorded from the restatements of the parent's rule (tests/vectorcheck.py, tests/vectorcheck_noflux.py) -- not
# from the code under test: status words in order, and the indices of the joint->joint columns left open.
UNIQUE_RECORDED = {
    "valid": ((32, 0, 0, 0, 0, 16, 0), []),
    "invalid": ((34, 0, 0, 0, 4, 17, 0), [0, 3, 9, 81]),
}


@pytest.mark.gpu
def test_links_unique_is_what_it_was(monkeypatch):
    """The default issues the parent's calls and no other -- neither new entry point is reached -- and gives its bits."""
    be_lib = _lib.load()
    called = []

    class Spy:
        def __getattr__(self, name):
            called.append(name)
            return getattr(be_lib, name)
    from graingraphnn_amd.backend import default_backend
    be = default_backend()
    monkeypatch.setattr(be, "lib", Spy())
    for name, (image, n_grain) in (("valid", tv.case("plain")[:2]), ("invalid", lens_image())):
        words, opened = UNIQUE_RECORDED[name]
        v = tv.restated(("unique", name), image, n_grain)
        assert tuple(v["status"][k] for k in vc.STATUS) == words and np.nonzero(v["jj"][1] == -1)[0].tolist() == opened
        dev = torch.from_numpy(image).to(DEV)
        for kw in ({}, dict(links="unique"), dict(links="unique", max_trace=3)):
            del called[:]
            got = vz.graph_from_image(dev, n_grain, strict=False, **kw)
            tv.assert_equals_restatement(got, v, name)
            assert [c for c in called if "junction" in c] == ["ggnn_image_junctions", "ggnn_junction_links"], called
            del called[:]
            res = vz.graphs_from_images(dev[None], [n_grain], strict=False, **kw)
            tu.assert_same_graph(vz.union_member(res, 0), got, name)
            assert [c for c in called if "junction" in c] == ["ggnn_image_junctions_traj", "ggnn_junction_links_traj"], called
            assert tuple(res["status"][0].values()) == words and tuple(res["status"][0]) == vc.STATUS
        del called[:]
        vz.graph_from_image(dev, n_grain, strict=False, links="trace")
        assert [c for c in called if "junction" in c] == ["ggnn_image_junction_windows_traj", "ggnn_junction_links_traj",
                                                          "ggnn_junction_links_trace_traj"], called


def same(t, a, what):
    a = np.ascontiguousarray(a)
    got = t.cpu().numpy()
    assert got.shape == a.shape and got.dtype == a.dtype, (what, got.shape, a.shape, got.dtype, a.dtype)
    assert np.array_equal(got.view(np.uint32) if a.dtype == np.float32 else got, a.view(np.uint32) if a.dtype == np.float32 else a), what


def sequence_samples(links):
    def make():
        d = frames()
        return vz.frames_to_samples(torch.from_numpy(d["frames"].astype(np.int32)).to(DEV), d["theta_x"], d["theta_z"], float(d["G"]),
                                    float(d["R"]), patch_pixels=501 * 501, extra_volume=d["extra_volume"], grid="points", links=links)
    return cached(("sequence", links), make)


@pytest.mark.gpu
def test_the_recorded_sequence_keeps_the_pairs_around_the_lens():
    d = frames()
    u = traced_union("nine frames", list(d["frames"].astype(np.int32)), [118] * 9, "periodic", grid="points")
    r = cached("nine frames tracked", lambda: tk.track(u, 118, "periodic", patch_pixels=501 * 501, extra_volume=d["extra_volume"]))
    assert r["pairs"] == [(t, t + 1) for t in range(8)] and [s["n_joint"] for s in u["status"]][6:] == [200, 176, 160]
    samples, report = sequence_samples("trace")
    assert len(samples) == 8 and report["pairs"] == r["pairs"] and report["skipped"] == []
    assert report["status"] == statuses(u) and [s["n_traced"] for s in report["status"]] == [0] * 6 + [4, 0, 0]
    assert all(vz.status_is_valid(s) for s in report["status"])
    plain, plain_report = sequence_samples("unique")
    # the present rule loses the two pairs around frame 36 (frame index 6) and names it: six of the eight pairs are left, the
    # five before it and (42, 48), which comes without its history
    assert len(plain) == 6 and plain_report["pairs"] == r["pairs"][:5] + [(7, 8)]
    assert [s[:2] for s in plain_report["skipped"]] == [(5, 6), (6, 7)] and all("frame 6" in s[2] for s in plain_report["skipped"])
    assert not plain[5][0]["grain"][:, 10].any() and not plain[5][0]["joint"][:, 6:8].any()
    for k in ("grain", "joint", "edge_event", "grain_event"):
        assert torch.equal(plain[5][3][k], samples[7][3][k]), k
    assert all(set(s) == set(vz.STATUS_WORDS) for s in plain_report["status"]) and plain_report["status"][6]["n_open_pairs"] == 4
    for t in range(5):                                          # the first five: bit-equal to links="unique"'s
        for a, b in zip(samples[t], plain[t]):
            assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a), t
        assert report["counts"][t] == plain_report["counts"][t]
    for t, (x, ei, ea, y, mask) in enumerate(samples):          # all eight: the tracker's restatement fed the traced union
        wy, wm, (h_area, h_extra, h_joint) = tk.cut(r, 118, t)
        for k in wy:
            same(y[k], wy[k], (t, "y", k))
        for k in wm:
            same(mask[k], wm[k], (t, "mask", k))
        same(x["grain"][:, 10], h_area, t), same(x["grain"][:, 4], h_extra, t), same(x["joint"][:, 6:8].contiguous(), h_joint, t)
        assert report["counts"][t] == r["counts"][t], t
        j0, j1 = r["joint_off"][t], r["joint_off"][t + 1]
        own = u["jj"][:, 3 * j0:3 * j1] - j0
        assert np.array_equal(ei[JJ].cpu().numpy(), own) and (own >= 0).all(), t
        recorded = {int(g) for f, g in zip(d["event_frame"], d["event_grain"]) if 6 * t + 1 <= f <= 6 * t + 6}
        assert set((torch.nonzero(y["grain_event"]).reshape(-1) + 1).tolist()) == recorded, t
    # the lens: its two junctions share a triple, so the pair (36, 42) counts them as ambiguous and leaves them unmatched
    assert report["counts"][6]["n_ambiguous"] == 2 and 26 in (torch.nonzero(samples[6][3]["grain_event"]).reshape(-1) + 1).tolist()
    lens = [j for j in range(200) if u["triples"][r["joint_off"][6] + j].tolist() == [25 + 6 * 118, 85 + 6 * 118, 94 + 6 * 118]]
    assert lens == [97, 101] and not samples[6][4]["joint"][lens].any()
    # the history columns of the pair (42, 48) are there: the pair (36, 42) was emitted
    x7 = samples[7][0]
    assert int((x7["grain"][:, 10] != 0).sum()) > 50 and int((x7["joint"][:, 6:8] != 0).any(1).sum()) > 100


@pytest.mark.gpu
def test_traced_samples_through_the_device_dataset_and_one_loss_each():
    from graingraphnn_amd import training
    samples, _ = sequence_samples("trace")
    R, Cm = product_models(10020, 1.0, DEV)
    R.train(), Cm.train()
    ds = training.DeviceDataset(samples, 2)
    db = training.DeviceBatches(ds)
    ds.set_order(np.array([6, 7, 0, 1, 2, 3, 4, 5]))            # the two pairs around the lens first
    db.next()
    assert list(ds.batch_ids(0)) == [6, 7]
    for i, sl in zip(ds.batch_ids(0), ds.slices(0)):
        x, ei, ea, y, mask = samples[i]
        a, b = sl[JJ]
        assert torch.equal(db.y_dict["edge_event"][a:b], y["edge_event"]), i
        a, b = sl["joint"]
        assert torch.equal(db.y_dict["joint"][a:b], y["joint"]) and torch.equal(db.mask["joint"][a:b].reshape(-1, 1), mask["joint"]), i
    lr = training.regressor_loss(db.y_dict, R(db.x_dict, db.edge_index_dict, db.edge_attr), db.mask, rows=db.rows)
    lc = training.classifier_loss(db.y_dict, Cm(db.x_dict, db.edge_index_dict, db.edge_attr), 1.0)
    assert bool(torch.isfinite(lr)) and bool(torch.isfinite(lc)) and float(lr.detach()) > 0 and float(lc.detach()) > 0


def forwards_and_a_step(image, n_grain, boundary, what, **kw):
    """sample_from_image(links="trace"): one regressor and one classifier forward through the drop-in models against the oracle
    at the project's parity bar, and one GrainRollout.step() with finite outputs."""
    from graingraphnn_amd import GrainRollout
    rs = np.random.RandomState(5)
    theta_x, theta_z = rs.uniform(0, np.pi / 2, n_grain), rs.uniform(0, np.pi / 2, n_grain)
    dev = torch.from_numpy(image).to(DEV)
    with pytest.raises(ValueError, match="n_open_pairs"):
        vz.sample_from_image(dev, theta_x, theta_z, 2.0, 0.4, span=6, boundary=boundary, **kw)
    X, EI, EA = vz.sample_from_image(dev, theta_x, theta_z, 2.0, 0.4, span=6, boundary=boundary, links="trace", **kw)
    assert int((EI[JJ] < 0).sum()) == 0 and all(bool(torch.isfinite(t).all()) for t in list(X.values()) + list(EA.values()))
    R, Cm = product_models(10020, 1.0, DEV)
    oR, oC = oracle_models(10020, 1.0)
    cpu = lambda d: {k: t.detach().cpu().clone() for k, t in d.items()}
    with torch.no_grad():
        yr, yc = R(X, EI, EA), Cm(X, EI, EA)
        oyr, oyc = oR(cpu(X), cpu(EI), cpu(EA)), oC(cpu(X), cpu(EI), cpu(EA))
        for k in ("joint", "grain", "grain_area"):
            assert_close(yr[k], oyr[k], f"{what} regressor {k}")
        for k in ("edge_event", "edge"):
            assert_close(yc[k], oyc[k], f"{what} classifier {k}")
        extra = dict(boundary="noflux", max_y=vz.image_max_y(image.shape[1], image.shape[0], kw.get("grid", "cells"))) if boundary == "noflux" else {}
        ro = GrainRollout(R, Cm, X, EI, EA, 6, refresh_centres=True, **extra)
        pred = ro.step()
        assert all(bool(torch.isfinite(t).all()) for t in pred.values()) and not ro.range_exceeded()
        assert all(bool(torch.isfinite(t).all()) for t in ro.x.values())
    return X, EI


@pytest.mark.gpu
def test_frame_36_into_the_models_and_a_rollout_step():
    d = frames()
    image = d["frames"][6].astype(np.int32)
    v = traced("frame 36", image, 118, grid="points")
    X, EI = forwards_and_a_step(image, 118, "periodic", "frame 36", grid="points", patch_pixels=501 ** 2)
    assert np.array_equal(EI[JJ].cpu().numpy(), v["jj"]) and X["joint"].shape == (200, 8)
    # the two-sided grain and its doubled column are plain list entries: junctions 97 and 101 are linked twice
    assert EI[JJ][1, 3 * 97:3 * 97 + 3].tolist() == [101, 101, 93] and int((EI[GJ][0] == 25).sum()) == 2


@pytest.mark.gpu
def test_the_band_into_the_models_and_a_noflux_rollout_step():
    image, n_grain = band_image()
    X, EI = forwards_and_a_step(image, n_grain, "noflux", "band")
    assert np.array_equal(EI[JJ].cpu().numpy(), traced("band", image, n_grain, "noflux", grid="cells")["jj"])
