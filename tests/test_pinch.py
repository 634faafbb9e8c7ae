"""Pinch windows read as necks (vectorize's pinch="neck"; the _pinch_traj entry points of include/ggnn.h) against the restatement
of tests/pinchcheck.py.

What the rule is for.  A pinch window is a 2 x 2 window with three distinct ids whose repeated id sits on a diagonal, [a b; c a]
or [b a; a c]: grain a runs through the pixel corner as a neck one pixel wide, and the grains b and c do not meet.  The
junction rule gives the window the key {a, b, c}, one junction too many for Euler's formula, and so calls invalid what a
drifting cell edge shorter than a pixel looks like in an image.  With such a window carrying no key the image is the valid
structure it is, with no pixel changed and no grain renumbered.

The CPU tests pin the restatement: on the figures measured with it before the kernels existed (a Voronoi sequence whose seeds
drift by a fraction of a pixel a frame, tools/vectorize_cost.py's `lattice_frames`; the rasters of the generator's structures),
on every image the vectorise tests call valid (nothing changes where there is no pinch window), on hand-drawn windows of both
diagonals, on a pinch window that the junction rule merges into a real junction (the count stays, m and the position change),
and on a grain with a pixel a knight's move from its body (not even corner-connected: it stays invalid).  The GPU tests hold
the kernels to the restatement bit for bit: xy, triples, the edge lists, rep, every status word, n_pinch_windows and the trace
counters, with canaries round every output of the entry points."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import pinchcheck as pk
import test_trace_links as tl
import test_vectorize as tv
import test_vectorize_union as tu
import tracecheck as tc
import trackcheck as tk
import vectorcheck as vc
import vectorcheck_noflux as vn
import vectorcheck_union as vu
from helpers import ROOT, assert_close, oracle_models, product_models
from graingraphnn_amd import _lib
from graingraphnn_amd import vectorize as vz
from graingraphnn_amd.synthetic import EDGE_TYPES

DEV = "cuda"
GJ, JG, JJ = EDGE_TYPES
W = 7
C = len(tc.COUNTERS)
cached = tv.cached


def necked(key, image, n_grain, boundary="periodic", pinch="neck", **kw):
    """The restatement of a named image under `pinch`, computed once and left unchanged."""
    return cached(("pinch", key, boundary, pinch, tuple(sorted(kw.items()))),
                  lambda: pk.vectorize(image, n_grain, boundary=boundary, pinch=pinch, **kw))


def necked_union(key, images, n_grains, boundary="periodic", **kw):
    return cached(("pinch union", key, boundary, tuple(sorted(kw.items()))),
                  lambda: pk.vectorize_union(images, n_grains, boundary=boundary, **kw))


def valid(v, boundary="periodic"):
    return pk.is_valid(v["status"], boundary)


# ---- the images --------------------------------------------------------------------------------------------------------------

def lattice(seed, size, T=64):
    """tools/vectorize_cost.py --track's sequence, made on the host: [T, size, size] int32, 121 grains."""
    def make():
        spec = importlib.util.spec_from_file_location("vectorize_cost", os.path.join(ROOT, "tools", "vectorize_cost.py"))
        cost = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(cost)
        frames = cost.lattice_frames(T, size, seed, "cpu").numpy().astype(np.int32)
        frames.setflags(write=False)
        return frames
    return cached(("lattice", seed, size, T), make)


def voronoi(ny, nx, seed, frame, boundary="periodic", n_side=4):
    """trackcheck.moving_seeds' Voronoi image: ids from 1 on the torus, from 2 between walls."""
    seeds = tk.moving_seeds(ny, nx, n_side, 3, seed)[frame]
    return tk.voronoi(seeds, ny, nx) if boundary == "periodic" else tk.voronoi(seeds, ny, nx, periodic=False, first_id=2)


# name -> (ny, nx, seed, frame, boundary): invalid under the junction rule, valid with the pinch window as a neck
REPAIRED = {"32 x 32, seed 13": (32, 32, 13, 0, "periodic"), "32 x 32, seed 25": (32, 32, 25, 0, "periodic"),
            "24 x 40, seed 48": (24, 40, 48, 2, "periodic"), "24 x 40, seed 49": (24, 40, 49, 0, "periodic"),
            "walls 32 x 32, seed 13": (32, 32, 13, 0, "noflux")}
TURNS = {"as drawn": lambda a: a, "transposed": lambda a: a.T, "mirrored": lambda a: a[:, ::-1]}


def repaired(name, turn="as drawn"):
    """-> (image, n_grain, boundary)"""
    ny, nx, seed, frame, boundary = REPAIRED[name]
    image = np.ascontiguousarray(TURNS[turn](voronoi(ny, nx, seed, frame, boundary))).astype(np.int32)
    return image, int(image.max()), boundary


def rolled_to_the_wrap():
    """32 x 32, seed 13, rolled so that its pinch window (8, 16) is window (31, 31): its TR, BL and BR are wrapped pixels."""
    image, n, _ = repaired("32 x 32, seed 13")
    return np.ascontiguousarray(np.roll(image, (23, 15), (0, 1))), n


def wide(x):
    """264 x 264, periodic, 11 x 11 seeds, seed 7 (frame 0), found on the CPU: of the seeds 0 .. 59 the first whose image the
    junction rule calls invalid and the neck rule valid (seeds 24, 31, 32, 47 and 48 are the others).  Its one pinch window
    (0, 140) is rolled to column x: 255 is the last thread of the first block of the count and emit passes, 256 the first thread
    of the second."""
    image = voronoi(264, 264, 7, 0, n_side=11).astype(np.int32)
    assert pk.pinch_windows(image, 121) == [(0, 140)]
    return np.ascontiguousarray(np.roll(image, x - 140, 1)), 121


def neck_and_lens():
    """16 x 16, no-flux, in the style of test_trace_links' `halves`: grain 2 left, grain 3 above grain 5 right, grain 4 a lens on
    the 2 | 3 boundary -- so four junctions hold the pair (2, 3) and every one of its columns is open --, and one pixel of grain 3
    at (9, 7) that hangs on its body through the corner alone: window (8, 7) = [2 3; 3 5] is a pinch window.  The walk from the
    lens down the 2 | 3 boundary reaches it, turns left with the boundary, goes round the pixel and ends at the junction
    {2, 3, 5} in window (9, 7): seven vertices."""
    img = np.full((16, 16), 2, np.int32)
    img[:, 8:] = 3
    img[2:5, 7] = 4
    img[9:, 8:] = 5
    img[9, 7] = 3
    return img


def neck_and_lens_on_a_torus():
    """32 x 32, periodic, 17 grains: test_vectorize's plain bricks with grain 17 as a lens of three pixels on the boundary of
    bricks 1 and 2 (rows 1 .. 3; test_trace_links' `lens_image` two rows higher), so that four junctions hold the pair (1, 2),
    and one pixel of brick 2 at (8, 7) that hangs on its brick through the corner alone: window (7, 7) = [1 2; 2 5] is a pinch
    window.  The walk from the lens down the 1 | 2 boundary reaches it after four vertices, turns left with the boundary and ends
    at the junction {1, 2, 5} in window (7, 6): five vertices.  Under the junction rule the pinch window carries {1, 2, 5} itself
    and the walk ends there, after four."""
    plain, n = tv.case("plain")[:2]
    img = plain.copy()
    img[1:4, 7] = n + 1
    img[8, 7] = 2
    return img, n + 1


TORUS = {"down a column": lambda: neck_and_lens_on_a_torus()[0], "along a row": lambda: np.ascontiguousarray(neck_and_lens_on_a_torus()[0].T),
         "the other diagonal": lambda: np.ascontiguousarray(neck_and_lens_on_a_torus()[0][:, ::-1])}
TRACED = {"down a column": lambda: neck_and_lens(), "along a row": lambda: np.ascontiguousarray(neck_and_lens().T),
          "the other diagonal": lambda: np.ascontiguousarray(neck_and_lens()[:, ::-1])}


def union_of_three():
    """128 x 128, 121 grains each: frame 19 of the drifting sequence (the neck rule repairs it), its frame 0 (no pinch window)
    and frame 56 of the sequence of seed 1 (a pixel a knight's move from its grain: it stays invalid)."""
    return [lattice(0, 128)[19], lattice(0, 128)[0], lattice(1, 128)[56]], [121, 121, 121]


# ---- CPU: the restatement ----------------------------------------------------------------------------------------------------

def test_the_predicate_on_windows_drawn_by_hand():
    assert pk.window_keys(1, 2, 3, 1, 3) == ([], False) and pk.is_pinch(1, 2, 3, 1, 3)          # [a b; c a]
    assert pk.window_keys(2, 1, 1, 3, 3) == ([], False) and pk.is_pinch(2, 1, 1, 3, 3)          # [b a; a c]
    for px in ((1, 1, 2, 3), (1, 2, 1, 3), (2, 1, 3, 1), (2, 3, 1, 1)):                         # the repeated id along an edge
        assert pk.window_keys(*px, 3) == vc.window_keys(*px, 3) == ([(0, 1, 2)], False) and not pk.is_pinch(*px, 3)
    assert pk.window_keys(1, 2, 3, 4, 4) == vc.window_keys(1, 2, 3, 4, 4) and pk.window_keys(1, 2, 3, 4, 4)[1]   # a quadruple
    assert pk.window_keys(1, 2, 2, 1, 2) == ([], False) and not pk.is_pinch(1, 2, 2, 1, 2)      # the two-id checkerboard
    assert not pk.is_pinch(1, 2, 3, 1, 2) and not pk.is_pinch(0, 2, 3, 0, 3)                    # an id outside [1, n_grain]
    before = (vc.window_keys, vn.window_keys, tc.window_keys)
    with pk.neck():
        assert vc.window_keys is vn.window_keys is tc.window_keys is pk.window_keys
    assert (vc.window_keys, vn.window_keys, tc.window_keys) == before
    with pk.neck("junction"):
        assert (vc.window_keys, vn.window_keys, tc.window_keys) == before
    with pytest.raises(ValueError, match="pinch must be"):
        with pk.neck("vertex"):
            pass
    # the frame the issue shows: grain 42's pixel in row 1 touches its body through the corner alone
    rows = np.array([[31, 31, 31, 32, 32], [41, 42, 32, 32, 32], [41, 41, 42, 42, 42]])
    assert [pk.is_pinch(rows[y, x], rows[y, x + 1], rows[y + 1, x], rows[y + 1, x + 1], 121) for y in (0, 1) for x in range(4)] == \
        [False, False, False, False, False, True, False, False]


@pytest.mark.parametrize("name", sorted(REPAIRED))
def test_small_voronoi_images_that_the_neck_rule_repairs(name):
    diagonals = set()
    for turn in TURNS:
        image, n, boundary = repaired(name, turn)
        a, b = necked((name, turn), image, n, boundary, "junction"), necked((name, turn), image, n, boundary)
        assert not valid(a, boundary) and valid(b, boundary), (name, turn)
        assert a["status"]["n_joint"] == b["status"]["n_joint"] + 1 and a["status"]["n_open_pairs"] == 7 and b["n_pinch_windows"] == 1
        (y, x), = pk.pinch_windows(image, n, boundary)
        tl_, tr, bl, br = tc.Windows(image, n, 2, boundary).pixels(y, x)
        diagonals.add("TL == BR" if tl_ == br else "TR == BL")
    assert diagonals == {"TL == BR", "TR == BL"}


def test_the_rolled_and_the_wide_images_hold_what_they_say():
    image, n = rolled_to_the_wrap()
    assert pk.pinch_windows(image, n) == [(31, 31)] and valid(necked("rolled", image, n)) and not valid(necked("rolled", image, n, pinch="junction"))
    for x in (255, 256):
        image, n = wide(x)
        assert pk.pinch_windows(image, n) == [(0, x)]
        a, b = necked(("wide", x), image, n, pinch="junction"), necked(("wide", x), image, n)
        assert not valid(a) and valid(b) and (a["status"]["n_joint"], b["status"]["n_joint"]) == (243, 242)


@pytest.mark.parametrize("seed,size,before,after,invalid", [(0, 128, 42, 64, []), (1, 128, 40, 63, [56]), (0, 96, 32, 63, [55]),
                                                            (0, 256, 60, 63, [47])])
def test_the_drifting_sequences(seed, size, before, after, invalid):
    """All 64 frames of every sequence of the table (no slice)."""
    frames = lattice(seed, size)
    assert int(frames.max()) == 121
    a = [necked(("lattice", seed, size, t), f, 121, pinch="junction") for t, f in enumerate(frames)]
    b = [necked(("lattice", seed, size, t), f, 121) for t, f in enumerate(frames)]
    assert sum(valid(v) for v in a) == before and sum(valid(v) for v in b) == after
    assert [t for t, v in enumerate(b) if not valid(v)] == invalid
    if (seed, size) == (0, 128):
        assert sum(v["status"]["n_joint"] for v in a) == 15516 and sum(v["status"]["n_joint"] for v in b) == 15488 == 64 * 242
        assert sum(v["n_pinch_windows"] for v in b) == 96
        assert [t for t in (17, 19, 21) if valid(a[t])] == [] and all(valid(a[t]) for t in (14, 15, 16, 18, 20))
        for links in ("unique", "trace"):                       # tracing repairs none of them, and breaks none
            ua = pk.vectorize_union(list(frames), [121] * 64, links=links, pinch="junction")
            ub = pk.vectorize_union(list(frames), [121] * 64, links=links)
            assert sum(vc.is_valid(s) for s in ua["status"]) == 42 and sum(vc.is_valid(s) for s in ub["status"]) == 64, links
            if links == "trace":
                continue
            ra, rb = tk.track(ua, 121, "periodic", shape=(128, 128)), tk.track(ub, 121, "periodic", shape=(128, 128))
            total = lambda r, k: sum(c[k] for c in r["counts"])
            assert len(ra["pairs"]) == 26 and len(rb["pairs"]) == 63
            assert [total(ra, k) for k in ("n_matched", "n_label0", "n_label1", "n_unlabelled")] == [5972, 17314, 292, 1270]
            assert [total(rb, k) for k in ("n_matched", "n_label0", "n_label1", "n_unlabelled")] == [14310, 41182, 848, 3708]
            assert total(rb, "n_ambiguous") == 0


def test_a_pixel_a_knights_move_from_its_grain_stays_invalid():
    """Frame 56 of the sequence of seed 1: one pixel of a grain is not even corner-connected to its body.  That is a
    disconnected grain, which no reading of a window mends."""
    image = lattice(1, 128)[56]
    v = necked(("lattice", 1, 128, 56), image, 121)
    assert not valid(v) and v["status"]["n_joint"] != 2 * v["status"]["n_present_grains"]
    lonely = []
    for g in range(1, 122):
        ys, xs = np.nonzero(image == g)
        for y, x in zip(ys, xs):
            around = image[np.ix_([(y - 1) % 128, y, (y + 1) % 128], [(x - 1) % 128, x, (x + 1) % 128])]
            if int((around == g).sum()) == 1 and len(ys) > 1:
                lonely.append((g, int(y), int(x)))
    assert len(lonely) == 1
    g, y, x = lonely[0]
    knight = [image[(y + dy) % 128, (x + dx) % 128] == g for dy, dx in ((1, 2), (2, 1), (-1, 2), (-2, 1), (1, -2), (2, -1), (-1, -2), (-2, -1))]
    assert any(knight)


@pytest.mark.parametrize("name,n_grain,size,n_pinch,n_joint,flips", [("generated_40_seed1", 115, 256, 1, 230, 7),
                                                                    ("generated_40_seed1", 115, 128, 1, 230, 11),
                                                                    ("generated_40_seed2", 117, 256, 3, 234, 4),
                                                                    ("generated_40_seed2", 117, 128, 2, 234, 4)])
def test_rasters_of_generated_structures_with_sub_pixel_edges(name, n_grain, size, n_pinch, n_joint, flips):
    image = tv.fixture_raster(name, size)
    a, b = necked((name, size), image, n_grain, pinch="junction"), necked((name, size), image, n_grain)
    assert a["status"]["n_joint"] == n_joint + 1 and a["status"]["n_open_pairs"] == 7 and not valid(a)
    assert b["status"]["n_joint"] == n_joint == 2 * n_grain and b["status"]["n_open_pairs"] == 0 and valid(b)
    assert b["n_pinch_windows"] == n_pinch
    ref, got = set(tv.reference_triples(tv.npz(name))), {tuple(t) for t in b["triples"].tolist()}
    print(f"{name} at {size}: {len(ref - got)} missing, {len(got - ref)} spurious; round trip {tv.round_trip(b, image, n_grain)[0]!r}")
    assert len(ref - got) == len(got - ref) == flips            # flips of edges shorter than a pixel: a triple lost, one gained


@pytest.mark.parametrize("name,size,n_pinch,n_joint", [("generated_80_seed7", 512, 4, 922), ("graph_120", 1024, 3, 2086)])
def test_valid_rasters_with_pinch_windows_stay_valid_with_the_same_count(name, size, n_pinch, n_joint):
    n_grain = tv.npz(name)["x_grain"].shape[0]
    image = tv.fixture_raster(name, size)
    a, b = tv.restated((name, size), image, n_grain), necked((name, size), image, n_grain)
    assert vc.is_valid(a["status"]) and valid(b) and a["status"]["n_joint"] == b["status"]["n_joint"] == n_joint
    assert b["n_pinch_windows"] == n_pinch and b["status"]["n_merged_windows"] == a["status"]["n_merged_windows"] - n_pinch


def test_images_without_a_pinch_window_come_out_as_they_were():
    """The recorded phase-field frames and every image the vectorise tests call valid: where there is no pinch window every
    array is equal under both modes.  The eleven with pinch windows are all of the kind the junction rule merges into a real
    junction: they stay valid, with the same junctions."""
    cases = dict(tl.valid_images())
    d = tl.frames()
    for i, t in enumerate(d["frame_ids"].tolist()):
        cases[f"recorded frame {t}"] = (d["frames"][i].astype(np.int32), 118, "periodic", dict(grid="points"))
    with_pinch, n_equal = [], 0
    for name, (image, n_grain, boundary, kw) in cases.items():
        one = vc.vectorize if boundary == "periodic" else vn.vectorize
        a, b = one(image, n_grain, **kw), pk.vectorize(image, n_grain, boundary=boundary, **kw)
        if not pk.is_valid(a["status"], boundary):
            # (the walls image read as a torus is no valid structure; frame 36 holds a lens, which links="trace" reads)
            assert name.startswith("stack periodic") or name == "recorded frame 36", name
            if name != "recorded frame 36":
                continue
        if pk.pinch_windows(image, n_grain, boundary):
            with_pinch.append(name)
            assert pk.is_valid(b["status"], boundary), name     # (the representative may move, and the numbering with it)
            assert sorted(map(tuple, a["triples"].tolist())) == sorted(map(tuple, b["triples"].tolist())), name
            assert a["status"]["n_merged_windows"] == b["status"]["n_merged_windows"] + b["n_pinch_windows"], name
            continue
        assert a["status"] == b["status"] and b["n_pinch_windows"] == 0, name
        for k in ("xy", "triples", "gj", "jj"):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (name, k)
        n_equal += 1
    assert sorted(with_pinch) == sorted(["generated_80 at 512", "graph_120 at 1024", "bricks: diagonal", "bricks: diagonal, radius 1",
                                         "bricks: seam", "stack periodic 32 x 32 [1]", "stack periodic 24 x 40 [1]"]
                                        + [f"noflux_40 at {s}, {g}" for s in (256, 128) for g in ("cells", "points")])
    assert n_equal >= 35
    assert all(f"recorded frame {t}" in cases for t in range(0, 49, 6)) and all(f"graph_40 at {s}" in cases for s in (96, 128, 256))


@pytest.mark.parametrize("seed", [6, 14])
def test_a_pinch_window_that_the_junction_rule_merges_into_a_real_junction(seed):
    """The pinch window lies within merge_radius of a window that really carries its key: the junction rule merges the two, so
    the count is the same under both modes and the image valid under both; the neck rule takes the window out of m, Sx, Sy."""
    image = tk.voronoi(tk.moving_seeds(32, 32, 4, 3, seed)[0], 32, 32)
    a, b = necked(("merged", seed), image, 16, pinch="junction"), necked(("merged", seed), image, 16)
    assert valid(a) and valid(b) and a["status"]["n_joint"] == b["status"]["n_joint"] == 32 and b["n_pinch_windows"] == 1
    assert a["status"]["n_merged_windows"] == b["status"]["n_merged_windows"] + 1
    (y, x), = pk.pinch_windows(image, 16)
    key = vc.window_keys(*tc.Windows(image, 16, 2, "periodic").pixels(y, x), 16)[0][0]
    at = lambda v: {tuple(t): v["xy"][j].tobytes() for j, t in enumerate(v["triples"].tolist())}   # (the numbering may move too)
    assert len(at(a)) == 32 and at(a).keys() == at(b).keys() and [k for k in at(a) if at(a)[k] != at(b)[k]] == [key]
    with pk.neck():
        Wb = tc.Windows(image, 16, 2, "periodic")
        m_neck = sum(key in Wb.keys(y + dy, x + dx) for dy in range(-4, 5) for dx in range(-4, 5))
    Wa = tc.Windows(image, 16, 2, "periodic")
    m_junction = sum(key in Wa.keys(y + dy, x + dx) for dy in range(-4, 5) for dx in range(-4, 5))
    assert m_junction == m_neck + 1 >= 2


@pytest.mark.parametrize("name", sorted(TRACED))
def test_hand_made_a_walk_through_a_pinch_vertex(name):
    image = TRACED[name]()
    (y, x), = pk.pinch_windows(image, 5, "noflux")
    px = tc.Windows(image, 5, 2, "noflux").pixels(y, x)
    assert sorted(px) == [2, 3, 3, 5] and (px[0] == px[3]) == (name == "the other diagonal")
    plain = necked(name, image, 5, "noflux")
    assert plain["status"]["n_joint"] == 6 and plain["status"]["n_open_pairs"] == 4 and not valid(plain, "noflux")
    v = necked(name, image, 5, "noflux", links="trace")
    assert valid(v, "noflux") and v["counters"] == dict(n_traced=4, n_trace_failed=0, n_trace_overflow=0)
    assert tl.assert_symmetric(v, plain["jj"][1]) == 4
    with pk.neck():
        T = tc.Tracer(tc.Windows(image, 5, 2, "noflux"), v["triples"], v["rep"])
        walks = sorted(T.partner(j, 1, 2, 100)[2] for j in range(6) if {1, 2} <= set(T.keys[j]))
    assert walks == [2, 2, 7, 7]                                # the lens's lower junction and {2, 3, 5}: through the pinch vertex
    # the junction rule stops those two walks at the pinch window: it carries {2, 3, 5}, and its owner is left by two exits
    w = necked(name, image, 5, "noflux", "junction", links="trace")
    assert w["counters"] == dict(n_traced=2, n_trace_failed=2, n_trace_overflow=0) and not valid(w, "noflux")


@pytest.mark.parametrize("name", sorted(TORUS))
def test_hand_made_a_walk_through_a_pinch_vertex_on_the_torus(name):
    """The periodic instantiation of the trace kernel is a body of its own: the same walk on a torus, down a column, along a row
    and with the other diagonal."""
    image = TORUS[name]()
    (y, x), = pk.pinch_windows(image, 17)
    px = tc.Windows(image, 17, 2, "periodic").pixels(y, x)
    assert sorted(px) == [1, 2, 2, 5] and (px[0] == px[3]) == (name == "the other diagonal")
    plain = necked(("torus", name), image, 17)
    assert plain["status"]["n_joint"] == 34 and plain["status"]["n_open_pairs"] == 4 and not valid(plain)
    v = necked(("torus", name), image, 17, links="trace")
    assert valid(v) and v["counters"] == dict(n_traced=4, n_trace_failed=0, n_trace_overflow=0)
    assert tl.assert_symmetric(v, plain["jj"][1]) == 4

    def walks(w):
        T = tc.Tracer(tc.Windows(image, 17, 2, "periodic"), w["triples"], w["rep"])
        return sorted(T.partner(j, 0, 1, 200)[2] for j in range(34) if {0, 1} <= set(T.keys[j]))
    with pk.neck():
        assert walks(v) == [1, 1, 5, 5]                         # up from the lens across the wrap; down through the pinch vertex
    assert walks(necked(("torus", name), image, 17, pinch="junction", links="trace")) == [1, 1, 4, 4]


def test_entry_points_validate_on_the_host():
    lib = _lib.load()
    assert lib.ggnn_version() == 26 == _lib.GGNN_ABI_VERSION
    names = {"ggnn_image_junctions_pinch_traj", "ggnn_image_junction_windows_pinch_traj", "ggnn_junction_links_trace_pinch_traj"}
    assert names <= set(_lib.EXPORTED_SYMBOLS)
    assert lib.ggnn_image_junctions_pinch_traj(None, 1, None, None) == -1
    assert lib.ggnn_image_junction_windows_pinch_traj(None, None, 1, None, None) == -1
    assert lib.ggnn_junction_links_trace_pinch_traj(None, 1, None) == -1
    buf = (ctypes.c_int64 * 64)()                 # (host memory: refused before anything would be launched)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def args(**kw):
        A = _lib.JunctionTrajArgs(p, p, p, p, p, p, p, p, 4 * 3 * 32, 32, 32, 3, 16, 8, 1.0, 1.0 / 32, 2, 0)
        A.images = None                           # (so that a call that passes every other check still launches nothing)
        for k, v in kw.items():
            setattr(A, k, v)
        return ctypes.byref(A)
    for mode in (_lib.GGNN_PINCH_JUNCTION, _lib.GGNN_PINCH_NECK):
        assert lib.ggnn_image_junctions_pinch_traj(args(), mode, p, None) == -1                        # (images NULL)
        assert lib.ggnn_image_junctions_pinch_traj(args(images=p), mode, None, None) == -1             # no counters
        assert lib.ggnn_image_junctions_pinch_traj(args(images=p), mode, p.value + 4, None) == -1      # counters not aligned
        assert lib.ggnn_image_junction_windows_pinch_traj(args(images=p), p, mode, None, None) == -1
        assert lib.ggnn_image_junction_windows_pinch_traj(args(images=p), p, mode, p.value + 4, None) == -1
        assert lib.ggnn_image_junction_windows_pinch_traj(args(images=p), None, mode, p, None) == -1   # no rep
        for bad in (dict(grain_off=None), dict(status=p.value + 4), dict(merge_radius=8), dict(nx=4), dict(n_grain=0),
                    dict(joint_capacity=0), dict(pitch=0.0), dict(boundary=2), dict(n_image=0), dict(workspace_bytes=4 * 96 - 1)):
            assert lib.ggnn_image_junctions_pinch_traj(args(images=p, **bad), mode, p, None) == -1, bad
            assert lib.ggnn_image_junction_windows_pinch_traj(args(images=p, **bad), p, mode, p, None) == -1, bad
    for mode in (-1, 2, 7):                       # no such mode, everything else in order
        assert lib.ggnn_image_junctions_pinch_traj(args(images=p), mode, p, None) == -1
        assert lib.ggnn_image_junction_windows_pinch_traj(args(images=p), p, mode, p, None) == -1

    def trace(mode, **kw):
        A = _lib.LinkTraceArgs(p, p, p, p, p, p, p, p, p, 32, 32, 3, 16, 8, 24, 128, 2, 0)
        A.images = None
        for k, v in kw.items():
            setattr(A, k, v)
        return lib.ggnn_junction_links_trace_pinch_traj(ctypes.byref(A), mode, None)
    assert trace(0) == -1 and trace(1) == -1
    for mode in (-1, 2):
        assert trace(mode, images=p) == -1
    for bad in (dict(rep=None), dict(counters=None), dict(status=p.value + 4), dict(n_image=0), dict(merge_radius=8), dict(nx=4),
                dict(boundary=2), dict(max_trace=0)):
        assert trace(1, images=p, **bad) == -1, bad


def test_header_binding_and_python_agree():
    src = open(os.path.join(ROOT, "include", "ggnn.h")).read()
    assert re.search(r"#define GGNN_ABI_VERSION 26\b", src)
    assert f"#define GGNN_PINCH_JUNCTION {_lib.GGNN_PINCH_JUNCTION}\n" in src and f"#define GGNN_PINCH_NECK {_lib.GGNN_PINCH_NECK}\n" in src
    assert f"#define GGNN_JUNCTION_STATUS_WORDS {W}\n" in src and len(vz.STATUS_WORDS) == W
    assert vz.PINCHES == {"junction": _lib.GGNN_PINCH_JUNCTION, "neck": _lib.GGNN_PINCH_NECK} and tuple(vz.PINCHES) == pk.PINCHES
    assert ctypes.sizeof(_lib.JunctionTrajArgs) == 9 * 8 + 5 * 8 + 4 * 4 and ctypes.sizeof(_lib.LinkTraceArgs) == 9 * 8 + 7 * 8 + 2 * 4


def python_calls():
    host = torch.ones(2, 8, 8, dtype=torch.int32)
    z = np.zeros(2)
    return (lambda **kw: vz.graph_from_image(host[0], 1, **kw), lambda **kw: vz.graphs_from_images(host, [1, 1], **kw),
            lambda **kw: vz.sample_from_image(host[0], z, z, 2.0, 0.4, span=6, **kw),
            lambda **kw: vz.samples_from_images(host, [z, z], [z, z], 2.0, 0.4, span=6, **kw),
            lambda **kw: vz.frames_to_samples(host, z, z, 2.0, 0.4, span=6, **kw),
            lambda **kw: vz.track_frames(host, 2, **kw))


def test_python_entry_points_take_the_keyword_and_refuse_another_value():
    for call in python_calls():
        for value in ("vertex", None, 1):
            with pytest.raises(ValueError, match="pinch must be 'junction' or 'neck'"):
                call(pinch=value)
            with pytest.raises(ValueError, match="pinch must be 'junction' or 'neck'"):
                call(pinch=value, links="trace")
        for kw in (dict(pinch="neck"), dict(pinch="junction"), dict(pinch="neck", links="trace")):
            with pytest.raises(_lib.GGNNError, match="device tensor"):   # (a host image gets as far as it did)
                call(**kw)


# ---- GPU: the kernels equal the restatement bit for bit ------------------------------------------------------------------------

def to_dev(images):
    return torch.from_numpy(np.stack(images).astype(np.int32)).to(DEV)


def statuses(v):
    """The restatement's status dicts as pinch="neck" returns them: the trace counters where it traced, then n_pinch_windows."""
    if isinstance(v["status"], dict):
        return dict(v["status"], **v.get("counters", {}), n_pinch_windows=v["n_pinch_windows"])
    counters = v.get("counters", [{}] * len(v["status"]))
    return [dict(s, **c, n_pinch_windows=p) for s, c, p in zip(v["status"], counters, v["n_pinch_windows"])]


def assert_single_equals(got, v, what):
    """graph_from_image(pinch="neck")'s result against pinchcheck.vectorize's."""
    xy, triples, ei, status = got[:4]
    assert status == statuses(v) and list(status) == list(statuses(v)), (what, status, statuses(v))
    assert np.array_equal(xy.cpu().numpy().view(np.uint32), v["xy"].view(np.uint32)) and xy.dtype == torch.float32, what
    assert np.array_equal(triples.cpu().numpy(), v["triples"]) and triples.dtype == torch.int32, what
    assert np.array_equal(ei[GJ].cpu().numpy(), v["gj"]) and np.array_equal(ei[JG].cpu().numpy(), v["gj"][::-1]), what
    assert np.array_equal(ei[JJ].cpu().numpy(), v["jj"]) and all(ei[et].dtype == torch.int64 and ei[et].is_contiguous() for et in EDGE_TYPES), what
    if len(got) > 4:
        assert got[4] == v["corner_grains"] and got[5] == float(v["max_y"]), what


def assert_union_equals(res, held, u, what):
    """graphs_from_images(pinch="neck")'s result and the arrays behind it against pinchcheck.vectorize_union's."""
    n = len(u["xy"])
    assert res["status"] == statuses(u), (what, res["status"], statuses(u))
    assert res["traj_offsets"]["grain"] == u["grain_off"] and res["traj_offsets"]["joint"] == [min(o, n) for o in u["joint_off"]]
    assert np.array_equal(res["xy"].cpu().numpy().view(np.uint32), u["xy"].view(np.uint32)), what
    assert np.array_equal(res["triples"].cpu().numpy(), u["triples"]), what
    ei = res["edge_index_dict"]
    assert np.array_equal(ei[GJ].cpu().numpy(), u["gj"]) and np.array_equal(ei[JG].cpu().numpy(), u["gj"][::-1]), what
    assert np.array_equal(ei[JJ].cpu().numpy(), u["jj"]), what
    assert np.array_equal(held["counts"].cpu().numpy(), u["counts"]), what
    if "rep" in u:
        assert held["rep"].dtype == torch.int32 and np.array_equal(held["rep"][:n].cpu().numpy(), u["rep"]) and not held["rep"][n:].any(), what
    if "corner_grains" in u:
        assert res["corner_grains"] == u["corner_grains"] and res["max_y"] == float(u["max_y"]), what


def run_union(images, n_grains, boundary, links="unique", **kw):
    return vz._graphs(to_dev(images), n_grains, kw.pop("grid", "cells"), kw.pop("merge_radius", 2), kw.pop("joint_capacity", None), False,
                      boundary, links, kw.pop("max_trace", None), "neck")


def check_image(key, image, n_grain, boundary, links="unique", grids=("cells", "points")):
    """One image through graph_from_image and through the one-image union, both grids, against the restatement."""
    dev = torch.from_numpy(image).to(DEV)
    for grid in grids:
        v = necked(key, image, n_grain, boundary, grid=grid, links=links)
        got = vz.graph_from_image(dev, n_grain, grid=grid, strict=False, boundary=boundary, links=links, pinch="neck")
        assert_single_equals(got, v, (key, grid))
        res, held = run_union([image], [n_grain], boundary, links, grid=grid)
        assert_union_equals(res, held, necked_union(key, [image], [n_grain], boundary, grid=grid, links=links), (key, grid))
        if valid(v, boundary):
            assert_single_equals(vz.graph_from_image(dev, n_grain, grid=grid, boundary=boundary, links=links, pinch="neck"), v, key)
        else:
            with pytest.raises(ValueError, match="n_pinch_windows"):
                vz.graph_from_image(dev, n_grain, grid=grid, boundary=boundary, links=links, pinch="neck")
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("turn", sorted(TURNS))
@pytest.mark.parametrize("name", sorted(REPAIRED))
def test_kernels_on_small_voronoi_images(name, turn):
    image, n_grain, boundary = repaired(name, turn)
    v = check_image((name, turn), image, n_grain, boundary)
    assert valid(v, boundary) and v["n_pinch_windows"] == 1
    with pytest.raises(ValueError, match="n_open_pairs': 7"):   # the default still refuses it, and says what it said
        vz.graph_from_image(torch.from_numpy(image).to(DEV), n_grain, boundary=boundary)


@pytest.mark.gpu
def test_kernels_with_the_pinch_window_across_the_periodic_wrap():
    image, n_grain = rolled_to_the_wrap()
    assert valid(check_image("rolled", image, n_grain, "periodic"))


@pytest.mark.gpu
@pytest.mark.parametrize("x", [255, 256])
def test_kernels_with_the_pinch_window_at_the_seam_of_two_blocks(x):
    image, n_grain = wide(x)
    v = check_image(("wide", x), image, n_grain, "periodic", grids=("cells",))
    assert valid(v) and v["status"]["n_joint"] == 242 and v["n_pinch_windows"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [6, 14])
def test_kernels_on_a_pinch_window_next_to_a_real_carrier(seed):
    image = tk.voronoi(tk.moving_seeds(32, 32, 4, 3, seed)[0], 32, 32).astype(np.int32)
    v = check_image(("merged", seed), image, 16, "periodic")
    dev = torch.from_numpy(image).to(DEV)
    xy, triples, _, status = vz.graph_from_image(dev, 16)
    xy_neck, triples_neck, _, status_neck = vz.graph_from_image(dev, 16, pinch="neck")
    at = lambda xy, triples: {tuple(t): p for t, p in zip(triples.tolist(), xy.view(torch.int32).tolist())}
    a, b = at(xy, triples), at(xy_neck, triples_neck)
    assert len(a) == 32 and a.keys() == b.keys() and sum(a[k] != b[k] for k in a) == 1 and valid(v)
    assert status["n_merged_windows"] == status_neck["n_merged_windows"] + 1 and status_neck["n_pinch_windows"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TRACED))
def test_kernels_walk_through_a_pinch_vertex(name):
    """Along a column and along a row: a walk turns with the image, and UP | DOWN and LEFT | RIGHT are separate code."""
    image = TRACED[name]()
    v = check_image(name, image, 5, "noflux", links="trace")
    assert v["counters"]["n_traced"] == 4 and valid(v, "noflux")
    plain = check_image(name, image, 5, "noflux")
    assert plain["status"]["n_open_pairs"] == 4


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TORUS))
def test_kernels_walk_through_a_pinch_vertex_on_the_torus(name):
    """The periodic neck instantiation of the trace kernel and its helpers, along a column and along a row."""
    image = TORUS[name]()
    v = check_image(("torus", name), image, 17, "periodic", links="trace")
    assert v["counters"] == dict(n_traced=4, n_trace_failed=0, n_trace_overflow=0) and valid(v)
    for limit in (4, 5):                                        # the walk through the pinch vertex reaches five vertices
        w = necked(("torus", name), image, 17, links="trace", max_trace=limit)
        assert w["counters"]["n_trace_overflow"] == (2 if limit == 4 else 0) and w["counters"]["n_traced"] == (2 if limit == 4 else 4)
        got = vz.graph_from_image(torch.from_numpy(image).to(DEV), 17, strict=False, links="trace", max_trace=limit, pinch="neck")
        assert_single_equals(got, w, (name, limit))
    assert check_image(("torus", name), image, 17, "periodic")["status"]["n_open_pairs"] == 4


def guarded_neck(images, n_grains, boundary, cap, trace, mode=_lib.GGNN_PINCH_NECK):
    """The _pinch_traj entry points on guarded arrays -> (xy, triples, gj, jj, status, counts, rep, counters, pinched), 16 guard
    words of -7 behind each (rep and counters: untouched without `trace`)."""
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
    pinched = torch.full((B + 16,), -7, dtype=torch.int64, device=DEV)
    counts = torch.full((n_total + 16,), -7, dtype=torch.int64, device=DEV)
    ws = torch.full((n_blocks + 16,), -7, dtype=torch.int32, device=DEV)
    A = _lib.JunctionTrajArgs(dev.data_ptr(), off.data_ptr(), counts.data_ptr(), xy.data_ptr(), triples.data_ptr(), gj.data_ptr(),
                              status.data_ptr(), ws.data_ptr(), 4 * n_blocks, nx, ny, B, n_total, cap, 1.0,
                              float(np.float32(1) / np.float32(nx)), 2, vz.BOUNDARIES[boundary])
    if trace:
        _lib.check(lib.ggnn_image_junction_windows_pinch_traj(ctypes.byref(A), rep.data_ptr(), mode, pinched.data_ptr(),
                                                              _lib.current_stream()), "windows")
    else:
        _lib.check(lib.ggnn_image_junctions_pinch_traj(ctypes.byref(A), mode, pinched.data_ptr(), _lib.current_stream()), "junctions")
    rows = gj[:6 * cap].view(2, 3 * cap)
    n = min(int(status[B * W + B]), cap)
    table = torch.stack([rows[1, :3 * n], rows[0, :3 * n]]).contiguous()          # joint -> grain, the junctions written
    csr = be.build_csr_batch([(table, cap, n_total)])[0]
    L = _lib.LinkTrajArgs(triples.data_ptr(), csr.rowptr.data_ptr(), csr.col.data_ptr(), jj.data_ptr(), status.data_ptr(),
                          n_total, cap, csr.col.numel(), B)
    _lib.check(lib.ggnn_junction_links_traj(ctypes.byref(L), _lib.current_stream()), "ggnn_junction_links_traj")
    if trace:
        T = _lib.LinkTraceArgs(dev.data_ptr(), off.data_ptr(), triples.data_ptr(), rep.data_ptr(), csr.rowptr.data_ptr(),
                               csr.col.data_ptr(), jj.data_ptr(), status.data_ptr(), counters.data_ptr(), nx, ny, B, n_total, cap,
                               csr.col.numel(), 4 * (nx + ny), 2, vz.BOUNDARIES[boundary])
        _lib.check(lib.ggnn_junction_links_trace_pinch_traj(ctypes.byref(T), mode, _lib.current_stream()), "trace")
    return xy, triples, gj, jj, status, counts, rep, counters, pinched


def assert_guarded_equals(out, u, B, cap, n_total, trace, what):
    xy, triples, gj, jj, status, counts, rep, counters, pinched = out
    n = min(cap, u["joint_off"][-1])
    words = status.tolist()
    assert [dict(zip(vz.STATUS_WORDS, words[b * W:(b + 1) * W])) for b in range(B)] == u["status"], what
    assert words[B * W:B * W + B + 1] == u["joint_off"] and words[B * W + B + 1:] == [-7] * 16, what
    assert pinched.tolist() == u["n_pinch_windows"] + [-7] * 16, (what, pinched.tolist())
    if trace:
        got = counters.tolist()
        assert [dict(zip(tc.COUNTERS, got[C * b:C * b + C])) for b in range(B)] == u["counters"] and got[C * B:] == [-7] * 16, what
        assert np.array_equal(rep[:n].cpu().numpy(), u["rep"]) and bool((rep[n:] == -7).all()), what
    else:
        assert bool((rep == -7).all()) and bool((counters == -7).all()), what
    assert np.array_equal(xy[:2 * n].cpu().numpy().view(np.uint32), u["xy"].reshape(-1).view(np.uint32)), what
    assert np.array_equal(triples[:3 * n].cpu().numpy(), u["triples"].reshape(-1)), what
    assert bool((xy[2 * n:] == -7).all()) and bool((triples[3 * n:] == -7).all()), what
    for lists, want in ((gj, u["gj"]), (jj, u["jj"])):
        rows = lists[:6 * cap].view(2, 3 * cap)
        assert np.array_equal(rows[:, :3 * n].cpu().numpy(), want), what
        assert bool((rows[:, 3 * n:] == -7).all()) and bool((lists[6 * cap:] == -7).all()), what
    assert np.array_equal(counts[:n_total].cpu().numpy(), u["counts"]) and bool((counts[n_total:] == -7).all()), what


@pytest.mark.gpu
@pytest.mark.parametrize("links", ["unique", "trace"])
def test_a_union_of_a_repaired_a_plain_and_an_invalid_image(links):
    """Each member equals its own call; then the entry points on guarded arrays, with room to spare and with a capacity that
    ends inside the first image, between the junctions in front of its pinch window and those behind it."""
    images, n_grains = union_of_three()
    u = necked_union("three", images, n_grains, links=links)
    assert [vc.is_valid(s) for s in u["status"]] == [True, True, False] and [p > 0 for p in u["n_pinch_windows"]] == [True, False, True]
    assert not vc.is_valid(necked(("lattice", 0, 128, 19), images[0], 121, pinch="junction")["status"])
    res, held = run_union(images, n_grains, "periodic", links)
    assert_union_equals(res, held, u, links)
    dev = to_dev(images)
    for t in range(3):
        own = vz.graph_from_image(dev[t], n_grains[t], strict=False, links=links, pinch="neck")
        tu.assert_same_graph(vz.union_member(res, t), own, (links, t))
    with pytest.raises(ValueError, match=r"1 of 3 images are not valid periodic.*image 2: \{.*'n_pinch_windows': [1-9]"):
        vz.graphs_from_images(dev, n_grains, links=links, pinch="neck")
    (y, x), = pk.pinch_windows(images[0], 121)[:1]
    cut = sum(1 for r in necked(("lattice", 0, 128, 19), images[0], 121, links="trace")["rep"] if r < y * 128 + x) + 1
    assert 1 < cut < u["joint_off"][1] - 1
    for cap in (u["joint_off"][3] + 5, cut):
        w = necked_union("three", images, n_grains, links=links, joint_capacity=cap)
        assert_guarded_equals(guarded_neck(images, n_grains, "periodic", cap, links == "trace"), w, 3, cap, sum(n_grains), links == "trace",
                              (links, cap))
    assert necked_union("three", images, n_grains, links=links, joint_capacity=cut)["status"][0]["overflow"] == 1


@pytest.mark.gpu
def test_a_no_flux_union_on_guarded_arrays():
    images = [repaired("walls 32 x 32, seed 13", turn)[0] for turn in ("as drawn", "mirrored")] + [neck_and_lens().repeat(2, 0).repeat(2, 1)]
    n_grains = [17, 17, 5]
    for links in ("unique", "trace"):
        u = necked_union("walls", images, n_grains, "noflux", links=links)
        assert u["n_pinch_windows"] == [1, 1, 1]
        cap = u["joint_off"][1] + 7
        w = necked_union("walls", images, n_grains, "noflux", links=links, joint_capacity=cap)
        assert_guarded_equals(guarded_neck(images, n_grains, "noflux", cap, links == "trace"), w, 3, cap, sum(n_grains), links == "trace", links)


@pytest.mark.gpu
def test_the_pinch_entry_points_in_junction_mode_are_their_namesakes():
    """GGNN_PINCH_JUNCTION through the new entry points: the plain restatement, and counters that the call zeroes."""
    images, n_grains = union_of_three()
    for trace in (False, True):
        plain = (tc.vectorize_union if trace else vu.vectorize)(images, n_grains, boundary="periodic")
        plain["n_pinch_windows"] = [0, 0, 0]
        cap = plain["joint_off"][3] + 5
        assert_guarded_equals(guarded_neck(images, n_grains, "periodic", cap, trace, _lib.GGNN_PINCH_JUNCTION), plain, 3, cap, sum(n_grains),
                              trace, trace)


@pytest.mark.gpu
def test_the_default_is_what_it_was(monkeypatch):
    """No keyword and pinch="junction" issue the parent's calls and no other and give equal bits: the restatement of the parent's
    rule, status dicts with the parent's words.  pinch="neck" reaches the _pinch_traj entry points, and they alone."""
    be_lib = _lib.load()
    called = []

    class Spy:
        def __getattr__(self, name):
            called.append(name)
            return getattr(be_lib, name)
    from graingraphnn_amd.backend import default_backend
    monkeypatch.setattr(default_backend(), "lib", Spy())
    image, n_grain, _ = repaired("32 x 32, seed 13")
    v = necked("32 x 32, seed 13 plain", image, n_grain, pinch="junction")
    traced = necked("32 x 32, seed 13 plain", image, n_grain, pinch="junction", links="trace")
    dev = torch.from_numpy(image).to(DEV)
    junction = lambda: [c for c in called if "junction" in c]
    for kw in ({}, dict(pinch="junction")):
        del called[:]
        got = vz.graph_from_image(dev, n_grain, strict=False, **kw)
        tv.assert_equals_restatement(got, v, "single")
        assert junction() == ["ggnn_image_junctions", "ggnn_junction_links"] and tuple(got[3]) == vc.STATUS
        del called[:]
        res = vz.graphs_from_images(dev[None], [n_grain], strict=False, **kw)
        tu.assert_same_graph(vz.union_member(res, 0), got, "union")
        assert junction() == ["ggnn_image_junctions_traj", "ggnn_junction_links_traj"] and tuple(res["status"][0]) == vc.STATUS
        del called[:]
        got = vz.graph_from_image(dev, n_grain, strict=False, links="trace", **kw)
        tl.assert_single_equals(got, traced, "trace")
        assert junction() == ["ggnn_image_junction_windows_traj", "ggnn_junction_links_traj", "ggnn_junction_links_trace_traj"]
        assert tuple(got[3]) == vc.STATUS + tc.COUNTERS
        del called[:]
        frames = torch.stack([dev, dev])
        res, nxt, prv = vz.track_frames(frames, n_grain, **kw)
        assert junction() == ["ggnn_image_junctions_traj", "ggnn_junction_links_traj", "ggnn_track_junctions"]
        assert all(tuple(s) == vc.STATUS for s in res["status"])
        _, report = vz.frames_to_samples(frames, np.zeros(n_grain), np.zeros(n_grain), 2.0, 0.4, span=6, **kw)
        assert set(report) == {"status", "pairs", "skipped", "counts"} and all(tuple(s) == vc.STATUS for s in report["status"])
    for links, want in (("unique", ["ggnn_image_junctions_pinch_traj", "ggnn_junction_links_traj"]),
                        ("trace", ["ggnn_image_junction_windows_pinch_traj", "ggnn_junction_links_traj", "ggnn_junction_links_trace_pinch_traj"])):
        for call in (lambda: vz.graph_from_image(dev, n_grain, links=links, pinch="neck"),
                     lambda: vz.graphs_from_images(dev[None], [n_grain], links=links, pinch="neck")):
            del called[:]
            call()
            assert junction() == want, called
    for call in python_calls():
        with pytest.raises(ValueError, match="pinch must be 'junction' or 'neck'"):
            call(pinch="vertex")


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", tu.BOUNDARIES)
def test_captured_graph_gives_the_same_bits(boundary, monkeypatch):
    """Vectorise + links + trace under "neck" in one captured graph, replayed twice: a replay starts from its own zeroed status,
    trace counters and pinch counters; all of them come back in the ONE read-back of the status tensor, which is counted on
    the public call: one `tolist`, and no other way to the host."""
    if boundary == "periodic":
        images, n_grains = [repaired("32 x 32, seed 13")[0], TORUS["down a column"](), TORUS["along a row"]()], [16, 17, 17]
    else:
        images = [repaired("walls 32 x 32, seed 13")[0], neck_and_lens().repeat(2, 0).repeat(2, 1), repaired("walls 32 x 32, seed 13", "mirrored")[0]]
        n_grains = [17, 5, 17]
    u = necked_union(("captured", boundary), images, n_grains, boundary, links="trace")
    assert sum(c["n_traced"] for c in u["counters"]) >= 4 and sum(u["n_pinch_windows"]) == 3
    dev = vz._stack(to_dev(images))
    off = vz.grain_offsets(n_grains, DEV)
    eager = vz._vectorize_union(dev, n_grains, "cells", 2, None, boundary, grain_off=off, links="trace", pinch="neck")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = vz._vectorize_union(dev, n_grains, "cells", 2, None, boundary, grain_off=off, links="trace", pinch="neck")
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for k in ("xy", "triples", "gj", "jj", "status", "counts", "rep"):
        assert torch.equal(held[k], eager[k]), k
    B = len(images)
    assert held["status"].numel() == B * W + B + 1 + (4 * B if boundary == "noflux" else 0) + C * B + B
    assert held["pinch_words"] == held["status"].numel() - B and held["trace_words"] == held["pinch_words"] - C * B
    res, _ = vz._graphs_of(held, held["status"].tolist(), False)
    assert_union_equals(res, held, u, boundary)
    reads = []
    for name in ("tolist", "cpu", "item", "numpy"):
        def counted(self, *a, _name=name, _real=getattr(torch.Tensor, name), **kw):
            reads.append(_name)
            return _real(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    public = vz.graphs_from_images(dev, n_grains, strict=False, boundary=boundary, links="trace", pinch="neck")
    monkeypatch.undo()
    assert reads == ["tolist"], reads
    assert public["status"] == statuses(u)


def forwards_and_a_step(image, n_grain, what):
    """sample_from_image(pinch="neck"): one regressor and one classifier forward through the drop-in models against the oracle at
    the project's parity bar, and one GrainRollout.step() with finite outputs."""
    from graingraphnn_amd import GrainRollout
    rs = np.random.RandomState(5)
    theta_x, theta_z = rs.uniform(0, np.pi / 2, n_grain), rs.uniform(0, np.pi / 2, n_grain)
    dev = torch.from_numpy(np.ascontiguousarray(image)).to(DEV)
    with pytest.raises(ValueError, match="n_open_pairs': 7"):
        vz.sample_from_image(dev, theta_x, theta_z, 2.0, 0.4, span=6)
    X, EI, EA = vz.sample_from_image(dev, theta_x, theta_z, 2.0, 0.4, span=6, pinch="neck")
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
        ro = GrainRollout(R, Cm, X, EI, EA, 6, refresh_centres=True)
        pred = ro.step()
        assert all(bool(torch.isfinite(t).all()) for t in pred.values()) and not ro.range_exceeded()
        assert all(bool(torch.isfinite(t).all()) for t in ro.x.values())
    return X, EI


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_grain,n_joint", [("generated_40_seed1", 115, 230), ("generated_40_seed2", 117, 234)])
def test_generated_rasters_into_the_models_and_a_rollout_step(name, n_grain, n_joint):
    for size in (256, 128):
        image = np.ascontiguousarray(tv.fixture_raster(name, size)).astype(np.int32)
        v = check_image((name, size), image, n_grain, "periodic", grids=("cells",))
        assert valid(v) and v["status"]["n_joint"] == n_joint
    X, EI = forwards_and_a_step(image, n_grain, f"{name} at 128")
    assert np.array_equal(EI[JJ].cpu().numpy(), v["jj"]) and X["joint"].shape == (n_joint, 8)


def same(t, a, what):
    a = np.ascontiguousarray(a)
    got = t.cpu().numpy()
    assert got.shape == a.shape and got.dtype == a.dtype, (what, got.shape, a.shape, got.dtype, a.dtype)
    assert np.array_equal(got.view(np.uint32) if a.dtype == np.float32 else got, a.view(np.uint32) if a.dtype == np.float32 else a), what


def drift_samples(pinch):
    def make():
        frames = torch.from_numpy(lattice(0, 128)[14:22].copy()).to(DEV)
        rs = np.random.RandomState(0)
        return vz.frames_to_samples(frames, rs.uniform(0, np.pi / 2, 121), rs.uniform(0, np.pi / 2, 121), 2.0, 0.4, span=6, pinch=pinch)
    return cached(("drift samples", pinch), make)


@pytest.mark.gpu
def test_frames_14_to_21_of_the_drifting_sequence_keep_every_pair():
    """Frames 17, 19 and 21 (here 3, 5 and 7) are invalid under the junction rule, which leaves one pair of seven."""
    frames = list(lattice(0, 128)[14:22])
    u = necked_union("frames 14 .. 21", frames, [121] * 8)
    r = cached("frames 14 .. 21 tracked", lambda: tk.track(u, 121, "periodic", shape=(128, 128)))
    assert r["pairs"] == [(t, t + 1) for t in range(7)] and all(vc.is_valid(s) for s in u["status"])
    samples, report = drift_samples("neck")
    assert report["pairs"] == r["pairs"] and report["skipped"] == [] and len(samples) == 7
    assert report["status"] == statuses(u) and report["n_pinch_windows"] == u["n_pinch_windows"]
    assert all(u["n_pinch_windows"][t] > 0 for t in (3, 5, 7))
    plain, plain_report = drift_samples("junction")
    assert plain_report["pairs"] == [(0, 1), (1, 2)] and [s[:2] for s in plain_report["skipped"]] == [(2, 3), (3, 4), (4, 5), (5, 6), (6, 7)]
    assert set(plain_report) == {"status", "pairs", "skipped", "counts"} and all(tuple(s) == vc.STATUS for s in plain_report["status"])
    # frames 14 and 15 hold no pinch window: the pair (14, 15) has the same bits, and so have the inputs of the pair (15, 16);
    # frame 16 holds one that the junction rule merges into a real junction, which moves under the neck rule, and the targets with it
    assert u["n_pinch_windows"][:3] == [0, 0, 1]
    for t, parts in ((0, 5), (1, 3)):
        for a, b in zip(samples[t][:parts], plain[t][:parts]):
            assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a), t
    assert report["counts"][0] == plain_report["counts"][0]
    for t, (x, ei, ea, y, mask) in enumerate(samples):          # all seven: the tracker's restatement fed the neck union
        wy, wm, (h_area, h_extra, h_joint) = tk.cut(r, 121, t)
        for k in wy:
            same(y[k], wy[k], (t, "y", k))
        for k in wm:
            same(mask[k], wm[k], (t, "mask", k))
        same(x["grain"][:, 10], h_area, t), same(x["grain"][:, 4], h_extra, t), same(x["joint"][:, 6:8].contiguous(), h_joint, t)
        assert report["counts"][t] == r["counts"][t], t
        j0, j1 = r["joint_off"][t], r["joint_off"][t + 1]
        own = u["jj"][:, 3 * j0:3 * j1] - j0
        assert np.array_equal(ei[JJ].cpu().numpy(), own) and (own >= 0).all(), t
        same(x["joint"][:, :2].contiguous(), u["xy"][j0:j1], (t, "xy"))
    res, nxt, prv = vz.track_frames(to_dev(frames), 121, pinch="neck")
    same(nxt, r["next"], "next"), same(prv, r["prev"], "prev")
    assert res["status"] == statuses(u)


@pytest.mark.gpu
def test_neck_samples_through_the_device_dataset_and_one_loss_each():
    from graingraphnn_amd import training
    samples, _ = drift_samples("neck")
    R, Cm = product_models(10020, 1.0, DEV)
    R.train(), Cm.train()
    ds = training.DeviceDataset(samples, 2)
    db = training.DeviceBatches(ds)
    ds.set_order(np.array([2, 3, 4, 5, 6, 0, 1]))               # the pairs the junction rule loses first
    db.next()
    assert list(ds.batch_ids(0)) == [2, 3]
    for i, sl in zip(ds.batch_ids(0), ds.slices(0)):
        x, ei, ea, y, mask = samples[i]
        a, b = sl[JJ]
        assert torch.equal(db.y_dict["edge_event"][a:b], y["edge_event"]), i
        a, b = sl["joint"]
        assert torch.equal(db.y_dict["joint"][a:b], y["joint"]) and torch.equal(db.mask["joint"][a:b].reshape(-1, 1), mask["joint"]), i
    lr = training.regressor_loss(db.y_dict, R(db.x_dict, db.edge_index_dict, db.edge_attr), db.mask, rows=db.rows)
    lc = training.classifier_loss(db.y_dict, Cm(db.x_dict, db.edge_index_dict, db.edge_attr), 1.0)
    assert bool(torch.isfinite(lr)) and bool(torch.isfinite(lc)) and float(lr.detach()) > 0 and float(lc.detach()) > 0
