"""A no-flux rollout's first state from a grain-ID image with walls (the GGNN_BC_NOFLUX mode of ggnn_image_junctions,
graingraphnn_amd.vectorize(boundary="noflux")) against the numpy restatement of tests/vectorcheck_noflux.py, and the
restatement against the reference's no-flux fixtures.

The contract.  KERNELS against RESTATEMENT: every output array, every status word, corner_grains and max_y equal, bit for bit.
RESTATEMENT against the REFERENCE: the fixtures' polygons (polycheck.restate, no-flux) filled into an image
(rastercheck.grain_image with the corner fill), vectorised.  Measured here with the restatement:

  raster                  status                                                   triples vs the fixture   round trip
  noflux_40_seed1, 256^2  valid: 198 junctions, 0 quadruple windows, 2 merged      4 missing / 4 spurious   0.0315094 (cells)
  noflux_40_seed1, 128^2  valid: 198 junctions, 2 quadruple windows, 3 merged      6 missing / 6 spurious   0.0639648 (cells)
  noflux_40_seed1,  96^2  invalid: 199 junctions, 7 open pairs                     --                       --
  noflux_80_seed3, 256^2  invalid: 805 junctions, 63 open pairs                    --                       --

Every missing / spurious triple is one T1 flip inside a set of four grains (an edge shorter than a pixel comes out with the
other diagonal): at 256^2 {0,65,68},{0,65,70} <-> {0,68,70},{65,68,70} and {1,30,32},{30,32,33} <-> {1,30,33},{1,32,33}.
The largest gap to the fixture's x_joint over the junctions with the fixture's triple is 2.0586 px ("cells") and 2.2468 px
("points") at 256^2, 2.0293 / 2.2261 px at 128^2.  The margin the rule implies is 3 px in each coordinate: the rasteriser
rounds a vertex to a lattice point (0.5), a window's position is the lattice point between its four pixels, at most half a
pixel from where either grid puts the vertex's pixel (0.5), and a position is the mean of carriers at offsets up to
merge_radius = 2 from the representative (2).  A round trip (image -> graph -> polygons -> image) moves a polygon side by
no more than its ends, so every pixel that differs lies within 4 whole pixels (3 px, rounded up once more by the
rasteriser) of a pixel at which the input changes id."""
import ctypes
import os

import numpy as np
import pytest
import torch

import polycheck as pc
import rastercheck as rc
import vectorcheck_noflux as vn
from helpers import GOLDEN, product_models
from graingraphnn_amd import _lib
from graingraphnn_amd import vectorize as vz
from graingraphnn_amd.synthetic import EDGE_TYPES

DEV = "cuda"
U32 = 2.0 ** -24
GAP_PIXELS = 3.0          # (the docstring: 0.5 + 0.5 + merge_radius)
NEAR_PIXELS = 4
CORNERS_40 = (39, 30, 10, 82)   # grain_image_cfg1.npz's noflux__corner_grains: the reference's traj.corner_grains
MEASURED_ROUND_TRIP = {("noflux_40_seed1", 256, "cells"): 0.0315093994140625, ("noflux_40_seed1", 256, "points"): 0.031158447265625,
                       ("noflux_40_seed1", 128, "cells"): 0.06396484375, ("noflux_40_seed1", 128, "points"): 0.0616455078125}
GJ, JG, JJ = EDGE_TYPES

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def npz(name):
    return cached(("npz", name), lambda: np.load(os.path.join(GOLDEN, name + ".npz")))


def reference_triples(d):
    """junction -> its sorted grain triple, for every junction of a fixture that has grains (noflux_80_seed3 carries two rows
    that no list names)."""
    t = {}
    for g, j in d["ei_grain__push__joint"].T:
        t.setdefault(int(j), []).append(int(g))
    return {j: tuple(sorted(g)) for j, g in sorted(t.items())}


def corner_grains_of(d):
    """The ids of the grains in the four corners of a no-flux fixture, in grain_image's order: the one grain that the wall
    junctions next to the corner on its two walls share beside grain 0."""
    triples, xy, max_y = reference_triples(d), d["x_joint"][:, :2], float(d["max_y"])
    walls = [j for j, t in triples.items() if t[0] == 0]

    def corner(cx, cy):
        a = min((j for j in walls if abs(xy[j, 0] - cx) < 2e-3), key=lambda j: abs(xy[j, 1] - cy))
        b = min((j for j in walls if abs(xy[j, 1] - cy) < 2e-3), key=lambda j: abs(xy[j, 0] - cx))
        (g,) = (set(triples[a]) & set(triples[b])) - {0}
        return g + 1
    return corner(0, 0), corner(1, 0), corner(0, max_y), corner(1, max_y)


def fixture_raster(name, s):
    """The fixture's polygons (restated) filled into an s x s no-flux image with its corner fill, computed once."""
    def make():
        d = npz(name)
        rowptr, col = pc.table_of(d["ei_joint__pull__grain"], d["x_grain"].shape[0])
        r = pc.restate(rowptr, col, d["x_joint"], boundary="noflux")
        img = rc.grain_image(rowptr, r["xy_sorted"], (s, s), "noflux", corner_grains=corner_grains_of(d))
        img.setflags(write=False)
        return img
    return cached(("raster", name, s), make)


def restated(key, image, n_grain, grid="cells", **kw):
    """The restatement of a named image, computed once and left unchanged."""
    return cached(("restated", key, grid, tuple(sorted(kw.items()))), lambda: vn.vectorize(image, n_grain, grid, **kw))


def round_trip(v, image, n_grain):
    """(share of differing pixels, the image) of the polygons of a vectorised no-flux image, rasterised again."""
    xj = np.zeros((len(v["xy"]), 8), np.float32)
    xj[:, :2] = v["xy"]
    rowptr, col = pc.table_of(v["gj"][::-1], n_grain)
    r = pc.restate(rowptr, col, xj, boundary="noflux")
    out = rc.grain_image(rowptr, r["xy_sorted"], (image.shape[1], image.shape[0]), "noflux", corner_grains=v["corner_grains"])
    return float((out != image).mean()), out


def flips(missing, spurious):
    """Pair the missing and the spurious triples off into T1 flips: two triples inside four grains against the two other
    triples inside the same four.  -> the sets of four, or an AssertionError naming the triple that no flip explains."""
    missing, spurious, out = set(missing), set(spurious), []
    while missing:
        a = min(missing)
        missing.discard(a)
        found = None
        for b in sorted(missing):
            four = set(a) | set(b)
            inside = sorted(s for s in spurious if set(s) <= four)
            if len(four) == 4 and len(inside) == 2 and set(inside[0]) | set(inside[1]) == four:
                found = (b, inside, four)
                break
        assert found is not None, f"no flip explains the missing triple {a}"
        missing.discard(found[0])
        spurious -= set(found[1])
        out.append(tuple(sorted(found[2])))
    assert not spurious, f"no flip explains the spurious triples {sorted(spurious)}"
    return sorted(out)


def near_a_boundary(image, reach):
    """Pixels within `reach` (Chebyshev) of a pixel whose right or lower neighbour, or the wall, ends its grain."""
    edge = np.zeros(image.shape, bool)
    edge[:, :-1] |= image[:, :-1] != image[:, 1:]
    edge[:, 1:] |= image[:, :-1] != image[:, 1:]
    edge[:-1] |= image[:-1] != image[1:]
    edge[1:] |= image[:-1] != image[1:]
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    for _ in range(reach):
        grown = edge.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ys, xs = slice(max(dy, 0), edge.shape[0] + min(dy, 0)), slice(max(dx, 0), edge.shape[1] + min(dx, 0))
                yd, xd = slice(max(-dy, 0), edge.shape[0] + min(-dy, 0)), slice(max(-dx, 0), edge.shape[1] + min(-dx, 0))
                grown[yd, xd] |= edge[ys, xs]
        edge = grown
    return edge


def assert_wall_junctions(v, nx, ny, valid):
    """Every junction with grain 0 in its triple lies on a wall with its normal coordinate exact; in a valid structure it has
    exactly two wall partners, the junctions it shares (0, a) and (0, b) with; no other junction holds grain 0."""
    triples, xy, max_y = v["triples"], v["xy"], v["max_y"]
    walls = np.nonzero(triples[:, 0] == 0)[0]
    assert not (triples[:, 1:] == 0).any()
    for j in walls:
        yr, xr = v["windows"][j]
        assert xr in (-1, nx - 1) or yr in (-1, ny - 1), (j, yr, xr)
        want_x = {-1: np.float32(0), nx - 1: np.float32(1)}.get(xr)
        want_y = {-1: np.float32(0), ny - 1: max_y}.get(yr)
        assert want_x is None or xy[j, 0] == want_x, (j, xy[j])
        assert want_y is None or xy[j, 1] == want_y, (j, xy[j])
        if valid:
            partners = v["jj"][1, 3 * j:3 * j + 2]          # the pairs (0, g1) and (0, g2)
            assert len(set(partners.tolist())) == 2 and all(triples[p, 0] == 0 for p in partners), (j, partners)
    assert (xy >= 0).all() and (xy[:, 0] <= 1).all() and (xy[:, 1] <= max_y).all()
    return walls


# ---- CPU: the restatement against the reference's fixtures ----------------------------------------------------------------

def test_the_reference_structure_fits_the_rule():
    """What the rule rests on, on both fixtures: three grains a junction, the wall junctions are those of grain 0, they lie
    on the walls, two are linked exactly when they share (0, a), and Euler's formula holds with grain 0 as the outer face."""
    for name, n_wall in (("noflux_40_seed1", 38), ("noflux_80_seed3", 65)):
        d = npz(name)
        triples = reference_triples(d)
        assert all(len(t) == 3 and len(set(t)) == 3 for t in triples.values())
        walls = {j for j, t in triples.items() if t[0] == 0}
        assert len(walls) == n_wall and len(triples) == 2 * (d["x_grain"].shape[0] - 1) - 2
        xy = d["x_joint"][sorted(walls), :2]
        assert (np.minimum(np.abs(xy), np.abs(xy - [1.0, float(d["max_y"])])).min(axis=1) < 1e-6).all()
        linked = {tuple(sorted((int(a), int(b)))) for a, b in d["ei_joint__connect__joint"].T if a in walls and b in walls
                  and len(set(triples[a]) & set(triples[b])) == 2 and (set(triples[a]) & set(triples[b])) >= {0}}
        by_pair = {}
        for j in walls:
            for g in triples[j][1:]:
                by_pair.setdefault(g, []).append(j)
        assert all(len(js) == 2 for js in by_pair.values())
        assert linked == {tuple(sorted(js)) for js in by_pair.values()}


@pytest.mark.parametrize("size,quads,merged,n_flips", [(256, 0, 2, 2), (128, 2, 3, 3)])
def test_rasters_of_noflux_40_give_its_graph_up_to_flips(size, quads, merged, n_flips):
    d, image = npz("noflux_40_seed1"), fixture_raster("noflux_40_seed1", size)
    assert corner_grains_of(d) == CORNERS_40 and not (image <= 1).any()
    by_joint = reference_triples(d)
    assert sorted(by_joint) == list(range(198))
    ref = [by_joint[j] for j in range(198)]
    at = {t: j for j, t in enumerate(ref)}
    for grid in ("cells", "points"):
        v = restated(("noflux_40", size), image, 101, grid)
        s = v["status"]
        assert vn.is_valid(s), s
        assert s == dict(n_joint=198, n_quad_windows=quads, n_merged_windows=merged, n_invalid_pixels=0, n_open_pairs=0,
                         n_present_grains=100, overflow=0), s
        assert v["corner_grains"] == CORNERS_40 and v["max_y"] == 1.0 and v["max_y"].dtype == np.float32
        got = [tuple(t) for t in v["triples"].tolist()]
        assert len(set(got)) == 198
        missing, spurious = set(ref) - set(got), set(got) - set(ref)
        fours = flips(missing, spurious)
        print(f"noflux_40 at {size}, {grid}: missing {sorted(missing)}, spurious {sorted(spurious)}, flips in {fours}")
        assert len(missing) == len(spurious) == 2 * n_flips and len(fours) == n_flips
        if size == 256:
            assert fours == [(0, 65, 68, 70), (1, 30, 32, 33)]
        walls = assert_wall_junctions(v, size, size, True)
        assert len(walls) == 37                               # (the fixture's 38: the flip {0,65,68},{0,65,70} has two)
        same = [(j, at[t]) for j, t in enumerate(got) if t in at]
        a, b = np.array([j for j, _ in same]), np.array([k for _, k in same])
        gap = np.abs(v["xy"][a].astype(np.float64) - d["x_joint"][b, :2]).max() * size
        share, out = cached(("round trip", size, grid), lambda: round_trip(v, image, 101))
        print(f"noflux_40 at {size}, {grid}: largest gap {gap:.4f} px, round-trip share {share!r}")
        assert gap <= GAP_PIXELS, gap
        assert not ((out != image) & ~near_a_boundary(image, NEAR_PIXELS)).any()
        assert share == MEASURED_ROUND_TRIP[("noflux_40_seed1", size, grid)], share   # (numpy on integers and fp32: exact)


@pytest.mark.parametrize("name,size,n_grain,n_joint,n_open", [("noflux_40_seed1", 96, 101, 199, 7),
                                                               ("noflux_80_seed3", 256, 400, 805, 63)])
def test_sub_pixel_edges_are_reported_not_repaired(name, size, n_grain, n_joint, n_open):
    """The negative cases: edges shorter than a pixel leave a raster that is no valid structure, and the status says so."""
    image = fixture_raster(name, size)
    v = restated((name, size), image, n_grain)
    s = v["status"]
    assert not vn.is_valid(s) and s["n_joint"] == n_joint and s["n_open_pairs"] == n_open, s
    assert s["n_invalid_pixels"] == 0 and s["overflow"] == 0 and s["n_present_grains"] == n_grain - 1
    assert int((v["jj"][1] == -1).sum()) == n_open
    assert_wall_junctions(v, size, size, False)


# ---- hand-made images -----------------------------------------------------------------------------------------------------

def bands(ny, nx, edges, cuts):
    """Band r = the rows [edges[r], edges[r + 1]); in it a grain begins at x = 0 and at every x of cuts[r].  Ids from 2.
    -> (int32 [ny, nx], n_grain with the boundary grain counted)."""
    img, gid = np.zeros((ny, nx), np.int32), 1
    for r, c in enumerate(cuts):
        xs = [0] + list(c) + [nx]
        for x0, x1 in zip(xs[:-1], xs[1:]):
            gid += 1
            img[edges[r]:edges[r + 1], x0:x1] = gid
    return img, gid


def walls_image(ny, nx):
    """Three bands of two grains, cut at x = 12, 20 and 8: a T at each wall (two at the side walls), a grain in each corner.
        2 2 2 3 3 3 3 3
        4 4 4 4 4 5 5 5
        6 6 7 7 7 7 7 7"""
    return bands(ny, nx, [0, ny // 3, 2 * ny // 3 + (1 if ny == 32 else 0), ny], [[12], [20], [8]])


# The ten junctions of walls_image, by hand.  Windows (yr, xr) with B1 / B2 the first rows of bands 1 and 2:
#   (-1, 11)  (B1-1, -1)  (B1-1, 11)  (B1-1, 19)  (B1-1, nx-1)  (B2-1, -1)  (B2-1, 7)  (B2-1, 19)  (B2-1, nx-1)  (ny-1, 7)
WALLS_TRIPLES = [(0, 1, 2), (0, 1, 3), (1, 2, 3), (2, 3, 4), (0, 2, 4), (0, 3, 5), (3, 5, 6), (3, 4, 6), (0, 4, 6), (0, 5, 6)]
WALLS_PARTNERS = [1, 4, 2, 0, 5, 2, 0, 1, 3, 2, 4, 7, 0, 8, 3, 1, 9, 6, 5, 7, 9, 3, 6, 8, 4, 9, 7, 5, 8, 6]


def walls_positions(ny, nx, grid):
    """x and y of the ten in lattice units (window + off, by hand), then the rule's product; None = the wall's own value."""
    f = np.float32
    off, pitch = vn.grid_constants(nx, grid)
    b1, b2 = ny // 3, 2 * ny // 3 + (1 if ny == 32 else 0)
    max_y = f(f(f(ny - 2) + f(2) * off) / f(f(nx - 2) + f(2) * off))
    xs = [11, "low", 11, 19, "far", "low", 7, 19, "far", 7]
    ys = ["low", b1 - 1, b1 - 1, b1 - 1, b1 - 1, b2 - 1, b2 - 1, b2 - 1, b2 - 1, "far"]
    at = lambda w, far: f(0) if w == "low" else far if w == "far" else f(f(f(w) + off) + f(0)) * pitch
    return np.array([[at(x, f(1)), at(y, max_y)] for x, y in zip(xs, ys)], f), max_y


@pytest.mark.parametrize("ny,nx", [(32, 32), (24, 40)])
def test_a_t_at_every_wall_against_lists_written_by_hand(ny, nx):
    image, n_grain = walls_image(ny, nx)
    assert n_grain == 7
    for grid in ("cells", "points"):
        v = restated(("walls", ny, nx), image, n_grain, grid)
        assert v["status"] == dict(n_joint=10, n_quad_windows=0, n_merged_windows=0, n_invalid_pixels=0, n_open_pairs=0,
                                   n_present_grains=6, overflow=0) and vn.is_valid(v["status"])
        assert [tuple(t) for t in v["triples"].tolist()] == WALLS_TRIPLES
        assert v["jj"][1].tolist() == WALLS_PARTNERS and v["jj"][0].tolist() == [j for j in range(10) for _ in range(3)]
        assert v["gj"][0].tolist() == [g for t in WALLS_TRIPLES for g in t] and np.array_equal(v["gj"][1], v["jj"][0])
        assert v["corner_grains"] == (2, 3, 6, 7)                 # a grain in each corner, and no junction there
        want, max_y = walls_positions(ny, nx, grid)
        assert np.array_equal(v["xy"].view(np.uint32), want.view(np.uint32)), (grid, v["xy"], want)
        assert v["max_y"] == max_y and v["max_y"].dtype == np.float32
        assert_wall_junctions(v, nx, ny, True)
    f = np.float32
    assert vn.max_y_of(32, 32, "cells") == 1 and vn.max_y_of(32, 32, "points") == 1
    assert vn.max_y_of(40, 24, "cells") == f(24) / f(40) and vn.max_y_of(40, 24, "points") == f(23) / f(39)
    for grid in ("cells", "points"):
        assert vz.image_max_y(40, 24, grid) == float(vn.max_y_of(40, 24, grid)) and vz.image_max_y(32, 32, grid) == 1.0


def variant_cases():
    """name -> (image, n_grain, keywords, what the status must show, junctions that must be there as (triple, x, y) with x, y
    in pixels of the "cells" grid or a wall's name).  All on walls_image(32, 32); id 8 is a grain of its own."""
    base, _ = walls_image(32, 32)
    n = 8

    def put(*areas):
        img = base.copy()
        for ys, xs, gid in areas:
            img[ys, xs] = gid
        return img
    # four grains at one point of a wall -- the outside, 2, 3 and 8 under a one-pixel strip of 2 | 3 --: a window on a wall
    # holds two inside pixels, so no window sees four ids; the point comes out as two junctions one pixel apart
    across = put((slice(1, 10), slice(8, 16), 8))
    # a grain two pixels wide at the top wall on the 2 | 3 boundary: (0, 1, 7) and (0, 2, 7) two windows apart, both kept
    close = put((slice(0, 4), slice(11, 13), 8))
    # three pixels in the corner: (0, 1, 7) is carried on the top wall at (-1, 1) and on the left wall at (1, -1), offset
    # (2, -2): one junction at their mean, its y set by the top wall; grain 7 is left with one junction
    stair = put(([0, 0, 1], [0, 1, 0], 8))
    # a line of 8 one pixel wide at the top wall inside 2: (0, 1, 7) at (-1, 4) and (-1, 5), merged within the radius
    sliver = put((slice(0, 3), 5, 8))
    # a notch three pixels wide: grain 1 touches the top wall twice, (0, 1, 7) at (-1, 3) and (-1, 6) beyond the radius
    twice = put((slice(0, 3), slice(4, 7), 8))
    bad = put((3, 3, 1), (15, 5, 0), (25, 20, n + 1), (28, 28, -4))
    valid = dict(valid=True, n_invalid_pixels=0, n_open_pairs=0, overflow=0)
    return {
        "four grains at a wall": (across, n, {}, dict(valid, n_joint=12, n_quad_windows=0, n_merged_windows=0, n_present_grains=7),
                                  [((0, 1, 2), 12, "low"), ((1, 2, 7), 12, 1), ((1, 3, 7), 8, 10), ((2, 3, 7), 16, 10)]),
        "two junctions close on a wall": (close, n, {}, dict(valid, n_joint=12, n_merged_windows=0),
                                          [((0, 1, 7), 11, "low"), ((0, 2, 7), 13, "low"), ((1, 2, 7), 12, 4)]),
        "staircase into a corner": (stair, n, {}, dict(valid=False, n_joint=11, n_merged_windows=1, n_invalid_pixels=0),
                                    [((0, 1, 7), 1, "low")]),
        "sliver at a wall": (sliver, n, {}, dict(valid=False, n_joint=11, n_merged_windows=1), [((0, 1, 7), 5.5, "low")]),
        "sliver at a wall, radius 0": (sliver, n, dict(merge_radius=0), dict(valid=False, n_joint=12, n_merged_windows=0),
                                       [((0, 1, 7), 5, "low"), ((0, 1, 7), 6, "low")]),
        "a grain at one wall twice": (twice, n, {}, dict(valid=False, n_joint=12, n_merged_windows=0, n_invalid_pixels=0),
                                      [((0, 1, 7), 4, "low"), ((0, 1, 7), 7, "low")]),
        "invalid pixels": (bad, n, {}, dict(valid=False, n_invalid_pixels=4, n_joint=10, n_present_grains=6), []),
        "capacity one short": (base, 7, dict(joint_capacity=9), dict(valid=False, overflow=1, n_joint=10), []),
        "capacity to spare": (base, 7, dict(joint_capacity=500), dict(valid, n_joint=10), []),
    }


VARIANTS = ("four grains at a wall", "two junctions close on a wall", "staircase into a corner", "sliver at a wall",
            "sliver at a wall, radius 0", "a grain at one wall twice", "invalid pixels", "capacity one short", "capacity to spare")


def variant(name):
    cases = cached("variants", variant_cases)
    assert tuple(cases) == VARIANTS
    return cases[name]


@pytest.mark.parametrize("name", VARIANTS)
def test_restatement_on_hand_made_variants(name):
    image, n_grain, kw, want, junctions = variant(name)
    v = restated(("variant", name), image, n_grain, **kw)
    s = dict(v["status"], valid=vn.is_valid(v["status"]))
    assert {k: s[k] for k in want} == want, (name, s)
    have = [(tuple(t), float(x), float(y)) for t, (x, y) in zip(v["triples"].tolist(), v["xy"])]
    for triple, x, y in junctions:
        entry = (triple, 0.0 if x == "low" else x / 32, 0.0 if y == "low" else y / 32)
        assert entry in have, (name, entry, have)
    assert_wall_junctions(v, 32, 32, s["valid"])
    if not s["valid"] and s["overflow"] == 0 and s["n_invalid_pixels"] == 0:
        assert s["n_open_pairs"] > 0 and int((v["jj"][1] == -1).sum()) == s["n_open_pairs"]   # reported, slot by slot
    if name == "capacity one short":
        assert len(v["xy"]) == 9 and v["gj"].shape == (2, 27)
    if name == "invalid pixels":   # the four pixels void their windows and nothing else
        assert [tuple(t) for t in v["triples"].tolist()] == WALLS_TRIPLES


def strip(nx):
    """An 8-row strip nx wide, two bands, cut so that junctions fall into the last window of a row's first segment of
    nx + 1 windows (x = 254) wherever the strip is wide enough, next to it (x = 255), and onto the far wall."""
    return bands(8, nx, [0, 4, 8], [[c for c in (100, 255) if c < nx], [c for c in (50, 254, 256) if c < nx]])


@pytest.mark.parametrize("nx", [255, 256, 257])
def test_strips_across_the_segment_edge(nx):
    image, n_grain = strip(nx)
    v = restated(("strip", nx), image, n_grain)
    assert vn.is_valid(v["status"]) and v["status"]["n_merged_windows"] == 0, v["status"]
    xs = [x for _, x in v["windows"]]
    assert (3, nx - 1) in v["windows"] and xs.count(nx - 1) == 1                 # the far wall's T
    assert v["xy"][v["windows"].index((3, nx - 1))].tolist() == [1.0, float(np.float32(4) * (np.float32(1) / np.float32(nx)))]
    assert 254 in xs and (nx == 255 or 253 in xs or 255 in xs)
    assert_wall_junctions(v, nx, 8, True)


def test_positions_and_the_snap_follow_the_stated_order_of_operations():
    """One merged wall junction of two carriers, on a wall of a non-square image in the points grid: x from the stated
    sequence of fp32 operations, y the wall's value; and max_y's own sequence."""
    image, n_grain = walls_image(24, 40)
    image = image.copy()
    image[21:24, 5] = 8                                            # a sliver at the FAR y wall inside 6: windows (23, 4), (23, 5)
    f = np.float32
    for grid in ("cells", "points"):
        v = vn.vectorize(image, 8, grid)
        off, pitch = vn.grid_constants(40, grid)
        j = [tuple(t) for t in v["triples"].tolist()].index((0, 5, 7))
        max_y = f(f(f(22) + f(f(2) * off)) / f(f(38) + f(f(2) * off)))
        want = f(f(f(4) + off) + f(f(1) / f(2))) * pitch
        assert v["windows"][j] == (23, 4) and v["xy"][j].tolist() == [float(want), float(max_y)], (grid, v["xy"][j])
        assert max_y == (f(24) / f(40) if grid == "cells" else f(23) / f(39))


def test_entry_point_validates_the_boundary_and_its_workspace():
    lib = _lib.load()
    assert lib.ggnn_version() == 26 == _lib.GGNN_ABI_VERSION
    assert ctypes.sizeof(_lib.JunctionArgs) == 8 * 8 + 4 * 8 + 4 * 4
    assert _lib.JunctionArgs._fields_[-1] == ("boundary", ctypes.c_int32)
    assert _lib.JunctionArgs.boundary.offset == _lib.JunctionArgs.merge_radius.offset + 4
    buf = (ctypes.c_int64 * 64)()                 # (host memory: refused before anything would be launched)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(**kw):
        A = _lib.JunctionArgs(p, p, p, p, p, p, p, 4 * 64, 32, 32, 16, 8, 1.0, 1.0 / 32, 2, _lib.BC_NOFLUX)
        A.image = None                            # (so that a call that passes every other check still launches nothing)
        for k, v in kw.items():
            setattr(A, k, v)
        return lib.ggnn_image_junctions(ctypes.byref(A), None)
    for bad in (2, -1, 7):
        assert call(image=p, boundary=bad) == -1, bad
    # The workspace: one word a block of the no-flux grid, ny + 1 rows of segments of nx + 1 windows.  (That the exact size
    # is accepted takes a launch: test_nothing_is_written_beyond_the_capacity_or_the_junctions.)
    seg = _lib.GGNN_JUNCTION_SEGMENT
    for nx, segments in ((255, 1), (256, 2), (257, 2)):
        assert (nx + 1 + seg - 1) // seg == segments
        assert call(image=p, nx=nx, ny=8, workspace_bytes=4 * 9 * segments - 1) == -1, nx
        # a workspace that suffices for the periodic grid of the same image but not for the no-flux one
        assert call(image=p, nx=nx, ny=8, workspace_bytes=4 * 8 * ((nx + seg - 1) // seg)) == -1, nx


def test_python_entry_points_refuse_an_unknown_boundary():
    image = torch.ones(8, 8, dtype=torch.int32)
    for call in (lambda: vz.graph_from_image(image, n_grain=2, boundary="walls"),
                 lambda: vz.sample_from_image(image, np.zeros(2), np.zeros(2), 2.0, 0.4, span=6, boundary="walls"),
                 lambda: vz.status_is_valid(dict(zip(vz.STATUS_WORDS, (0,) * 7)), "walls")):
        with pytest.raises(_lib.GGNNError, match="boundary must be"):
            call()
    s = dict(zip(vz.STATUS_WORDS, (10, 0, 0, 0, 0, 6, 0)))
    assert vz.status_is_valid(s, "noflux") and not vz.status_is_valid(s) and not vz.status_is_valid(dict(s, n_joint=12), "noflux")
    assert vz.status_is_valid(dict(s, n_joint=12)) and vz.STATUS_WORDS == vn.STATUS
    for word in ("n_invalid_pixels", "n_open_pairs", "overflow"):
        assert not vz.status_is_valid(dict(s, **{word: 1}), "noflux"), word


# ---- GPU: the kernels equal the restatement bit for bit --------------------------------------------------------------------

def assert_equals_restatement(got, v, what):
    """got = graph_from_image(boundary="noflux")'s (xy, triples, edge_index_dict, status, corner_grains, max_y)."""
    xy, triples, ei, status, corners, max_y = got
    assert status == v["status"], (what, status, v["status"])
    assert corners == v["corner_grains"] and isinstance(max_y, float) and max_y == float(v["max_y"]), (what, corners, max_y)
    assert xy.dtype == torch.float32 and triples.dtype == torch.int32 and all(ei[et].dtype == torch.int64 for et in EDGE_TYPES)
    assert np.array_equal(triples.cpu().numpy(), v["triples"]), what
    assert np.array_equal(xy.cpu().numpy().view(np.uint32), v["xy"].view(np.uint32)), what
    assert np.array_equal(ei[GJ].cpu().numpy(), v["gj"]), what
    assert np.array_equal(ei[JG].cpu().numpy(), v["gj"][::-1]), what
    assert np.array_equal(ei[JJ].cpu().numpy(), v["jj"]), what
    assert all(ei[et].is_contiguous() for et in EDGE_TYPES)


def run_both_ways(image, n_grain, v, what, **kw):
    """strict=False equals the restatement; strict=True does too, or raises and names the rule, as the status decides."""
    dev_image = torch.from_numpy(np.array(image)).to(DEV)                    # (a copy: the cached rasters are read-only)
    assert_equals_restatement(vz.graph_from_image(dev_image, n_grain, strict=False, boundary="noflux", **kw), v, what)
    if vn.is_valid(v["status"]):
        assert_equals_restatement(vz.graph_from_image(dev_image, n_grain, boundary="noflux", **kw), v, what)
    else:
        with pytest.raises(ValueError, match=r"not a valid noflux grain structure.*n_joint == 2 n_present_grains - 2"):
            vz.graph_from_image(dev_image, n_grain, boundary="noflux", **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("ny,nx", [(32, 32), (24, 40)])
def test_kernels_on_the_walls_images(ny, nx):
    image, n_grain = walls_image(ny, nx)
    for grid in ("cells", "points"):
        run_both_ways(image, n_grain, restated(("walls", ny, nx), image, n_grain, grid), (ny, nx, grid), grid=grid)
    # the periodic reading of the same image is another graph, and its call returns what it always did
    assert len(vz.graph_from_image(torch.from_numpy(image).to(DEV), n_grain, strict=False)) == 4


@pytest.mark.gpu
@pytest.mark.parametrize("name", VARIANTS)
def test_kernels_on_hand_made_variants(name):
    image, n_grain, kw, _, _ = variant(name)
    run_both_ways(image, n_grain, restated(("variant", name), image, n_grain, **kw), name, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("nx", [255, 256, 257])
def test_kernels_on_strips_across_the_segment_edge(nx):
    image, n_grain = strip(nx)
    run_both_ways(image, n_grain, restated(("strip", nx), image, n_grain), nx)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [128, 256, 96])
def test_kernels_on_rasters_of_noflux_40(size):
    image = fixture_raster("noflux_40_seed1", size)
    run_both_ways(image, 101, restated(("noflux_40", size), image, 101), size)
    if size == 96:
        got = vz.graph_from_image(torch.from_numpy(image.copy()).to(DEV), 101, strict=False, boundary="noflux")
        assert int((got[2][JJ][1] == -1).sum()) == 7
        with pytest.raises(ValueError, match="n_open_pairs"):
            vz.sample_from_image(torch.from_numpy(image.copy()).to(DEV), np.zeros(101), np.zeros(101), 2.0, 0.4, span=6,
                                 boundary="noflux", strict=False)


@pytest.mark.gpu
def test_nothing_is_written_beyond_the_capacity_or_the_junctions():
    """The two entry points themselves on guarded arrays: capacity one short of the 10 junctions (overflow set), then four to
    spare; the four words behind the one status row keep their guard through both calls."""
    image, n_grain = walls_image(24, 40)
    lib, dev_image = _lib.load(), torch.from_numpy(image).to(DEV)
    from graingraphnn_amd.backend import default_backend
    counts = default_backend().image_compare(dev_image, None, n_grain)[1]
    for cap in (9, 14):
        v = restated(("walls", 24, 40, cap), image, n_grain, joint_capacity=cap)
        n = min(cap, 10)
        xy = torch.full((2 * cap + 16,), -7.0, dtype=torch.float32, device=DEV)
        triples = torch.full((3 * cap + 16,), -7, dtype=torch.int32, device=DEV)
        gj = torch.full((6 * cap + 16,), -7, dtype=torch.int64, device=DEV)
        status = torch.full((7 + 4,), -7, dtype=torch.int64, device=DEV)
        ws = torch.full((25 + 8,), -7, dtype=torch.int32, device=DEV)              # (ny + 1 rows of one segment)
        A = _lib.JunctionArgs(dev_image.data_ptr(), counts.data_ptr(), xy.data_ptr(), triples.data_ptr(), gj.data_ptr(),
                              status.data_ptr(), ws.data_ptr(), 4 * 25, 40, 24, n_grain, cap, 1.0,
                              float(np.float32(1) / np.float32(40)), 2, _lib.BC_NOFLUX)
        _lib.check(lib.ggnn_image_junctions(ctypes.byref(A), _lib.current_stream()), "ggnn_image_junctions")
        assert dict(zip(vn.STATUS, status[:7].tolist())) == dict(v["status"], n_open_pairs=0) and bool((status[7:] == -7).all())
        assert v["status"]["overflow"] == (1 if cap == 9 else 0) and bool((ws[25:] == -7).all())
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
        assert dict(zip(vn.STATUS, status[:7].tolist())) == v["status"] and bool((status[7:] == -7).all())
        cols = jj[:6 * cap].view(2, 3 * cap)
        assert np.array_equal(cols[:, :3 * n].cpu().numpy(), v["jj"])
        assert bool((cols[:, 3 * n:] == -7).all()) and bool((jj[6 * cap:] == -7).all())
        A.workspace_bytes = 4 * 24                                                  # enough for the periodic grid only
        assert lib.ggnn_image_junctions(ctypes.byref(A), _lib.current_stream()) == -1


@pytest.mark.gpu
def test_captured_graph_gives_the_same_bits():
    image, n_grain = walls_image(24, 40)
    v = restated(("walls", 24, 40), image, n_grain)
    dev_image = torch.from_numpy(image).to(DEV)
    eager = vz._vectorize(dev_image, n_grain, "cells", 2, None, "noflux")        # (also the warm-up of the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = vz._vectorize(dev_image, n_grain, "cells", 2, None, "noflux")
    for _ in range(2):                                                          # (a replay starts from its own zeroed status)
        graph.replay()
    torch.cuda.synchronize()
    for k in ("xy", "triples", "gj", "jj", "status"):
        assert torch.equal(held[k], eager[k]), k
    words = held["status"].tolist()
    assert dict(zip(vn.STATUS, words)) == v["status"] and tuple(words[7:]) == v["corner_grains"]
    assert np.array_equal(held["xy"][:10].cpu().numpy().view(np.uint32), v["xy"].view(np.uint32))


def host_sample(v, image, theta_x, theta_z, G, R, span, dev):
    """The sample of sample_from_image(boundary="noflux"), assembled on the host from the restatement: the graph, the
    features and the areas in numpy; centres and edge lengths by the calls the rollout itself refreshes them with."""
    from graingraphnn_amd.backend import default_backend
    from graingraphnn_amd.generator import feature_rows
    n_grain, n_joint = len(theta_x), len(v["xy"])
    fg, fj = feature_rows(theta_x, theta_z, n_joint, G, R, span)
    xg, xj = fg.astype(np.float32), fj.astype(np.float32)
    xj[:, :2] = v["xy"]
    xg[:, 3] = (rc.compare(image, None, n_grain)[1][1:] / float(image.size)).astype(np.float32)
    be = default_backend()
    X = {"grain": torch.from_numpy(xg).to(dev), "joint": torch.from_numpy(xj).to(dev)}
    EI = {GJ: torch.from_numpy(v["gj"].copy()).to(dev), JG: torch.from_numpy(v["gj"][::-1].copy()).to(dev),
          JJ: torch.from_numpy(v["jj"].copy()).to(dev)}
    csr = be.build_csr_batch([(EI[JG], n_joint, n_grain)])[0]
    be.grain_centres(csr, X["joint"], X["grain"], boundary="noflux")
    X["grain"][0] = torch.from_numpy(np.concatenate([[0.5, 0.5, 0, 0, 0], xg[0, 5:10], [0]]).astype(np.float32)).to(dev)
    EA = {et: torch.zeros(EI[et].size(1), 1, dtype=torch.float32, device=dev) for et in EDGE_TYPES}
    be.step_refresh(X["joint"], X["grain"], float("inf"), torch.zeros(2, dtype=torch.int32, device=dev),
                    [(EI[et], X[et[0]], X[et[2]], EA[et]) for et in EDGE_TYPES])
    return X, EI, EA, csr


@pytest.mark.gpu
@torch.no_grad()
def test_raster_of_noflux_40_into_a_noflux_rollout():
    """sample_from_image(boundary="noflux") on the 256^2 raster: the restatement's graph in the reference's layout; the
    rollout's boundary step finds nothing to change; three steps equal, bit for bit, those from the sample assembled on the
    host; and layer 0's grain image is the restated round trip of the input."""
    from graingraphnn_amd import GrainRollout
    from graingraphnn_amd.backend import default_backend
    d, image = npz("noflux_40_seed1"), fixture_raster("noflux_40_seed1", 256)
    v = restated(("noflux_40", 256), image, 101)
    rs = np.random.RandomState(5)
    theta_x, theta_z = rs.uniform(0, np.pi / 2, 101), rs.uniform(0, np.pi / 2, 101)
    theta_x[0] = theta_z[0] = np.pi / 4                                  # (the fixture's boundary grain)
    dev_image = torch.from_numpy(image.copy()).to(DEV)
    max_y = vz.image_max_y(256, 256, "cells")
    X, EI, EA = vz.sample_from_image(dev_image, theta_x, theta_z, 2.0, 0.4, span=6, boundary="noflux")
    assert {k: (tuple(t.shape), t.dtype) for k, t in X.items()} == {"grain": ((101, 11), torch.float32),
                                                                    "joint": ((198, 8), torch.float32)}
    assert np.array_equal(EI[GJ].cpu().numpy(), v["gj"]) and np.array_equal(EI[JJ].cpu().numpy(), v["jj"])
    assert np.array_equal(EI[JG].cpu().numpy(), v["gj"][::-1]) and int((EI[GJ][0] == 0).sum()) == 37   # the FULL lists
    xg, xj = X["grain"].cpu().numpy(), X["joint"].cpu().numpy()
    assert np.array_equal(xj[:, :2].view(np.uint32), v["xy"].view(np.uint32))
    assert np.array_equal(xg[0].view(np.uint32), d["x_grain"][0].view(np.uint32))          # the reference's boundary row
    HX, HEI, HEA, csr = host_sample(v, image, theta_x, theta_z, 2.0, 0.4, 6, DEV)
    for k in X:
        assert torch.equal(X[k], HX[k]), k
    for et in EDGE_TYPES:
        assert torch.equal(EA[et], HEA[et]) and EA[et].shape == (594, 1), et
    rowptr, col = pc.table_of(v["gj"][::-1], 101)
    r = pc.restate(rowptr, col, xj, boundary="noflux")
    assert np.abs(xg[1:, :2] - r["centre"][1:]).max() <= 2 * int(r["sides"][1:].max()) * 2 * U32
    # the rollout's own boundary step leaves the first state as it is
    bj, bg = X["joint"].clone(), X["grain"].clone()
    default_backend().noflux_boundary(csr, bj, bg, max_y=max_y)
    assert torch.equal(bj, X["joint"]) and torch.equal(bg, X["grain"])

    R, Cm = product_models(10020, 1.0, DEV)
    states = []
    for x, ei, ea in ((X, EI, EA), (HX, HEI, HEA)):
        ro = GrainRollout(R, Cm, x, ei, ea, 6, refresh_centres=True, boundary="noflux", max_y=max_y)
        ro.enable_polygons(capacity=3)
        seen = []
        for _ in range(3):
            pred = ro.step()
            assert all(bool(torch.isfinite(t).all()) for t in pred.values())
            seen.append({**{"pred " + k: t.clone() for k, t in pred.items()}, **{"x " + k: t.clone() for k, t in ro.x.items()}})
        assert not ro.range_exceeded()
        states.append((seen, ro))
    for a, b in zip(states[0][0], states[1][0]):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert not torch.equal(states[0][0][0]["x joint"], states[0][0][2]["x joint"])
    ro = states[0][1]
    layer0 = ro.grain_image((256, 256), layer=0, corner_grains=v["corner_grains"])
    share, want = cached(("round trip", 256, "cells"), lambda: round_trip(v, image, 101))
    assert np.array_equal(layer0.cpu().numpy(), want)
    error = ro.image_error(layer0, dev_image)
    assert error["differing"] == int((want != image).sum()) and error["rate"] == share == MEASURED_ROUND_TRIP[("noflux_40_seed1", 256, "cells")]
