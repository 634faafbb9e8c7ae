"""Labelling a STACK of equal-shaped maps in launches that do not grow with T (ggnn_label_grains_stack,
ggnn_label_orientations_stack; vectorize.label_maps / label_orientation_maps / samples_from_orientation_maps /
samples_from_euler_maps, and label_sequence / label_orientation_sequence on top of them).

The contract, by reference to the single-map rule: frame t's image, n_grains, means and nine status words are those of the
single call on frame t, BIT FOR BIT -- no tolerance anywhere.  Two oracles, both from before this file: the numpy restatements
tests/labelcheck.label and tests/orientcheck.label applied frame by frame, and the device's own single-map call applied
frame by frame.  The shapes are test_label.py's, the smallest that place every seam: 3 x 3, 15 x 65, 16 x 64, 33 x 127.

The tests aim at the places where a stack is not a taller image: counters of a wave whose lanes lie in several frames (3 x 3:
seven frames a wave), chunks and list stretches at a frame's end, sweep words per frame, the rank restarting per frame, the
wrap of a frame going to its own first row, a capacity that ends inside one frame's grains."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import labelcheck as lc
import orientcheck as oc
import test_label as tl
import test_orient as to
from helpers import GOLDEN, ROOT, product_models
from graingraphnn_amd import _lib
from graingraphnn_amd import vectorize as vz
from graingraphnn_amd.synthetic import EDGE_TYPES

DEV = "cuda"
BOUNDARIES = ("periodic", "noflux")
SHAPES = [(3, 3), (15, 65), (16, 64), (33, 127)]
DEPTHS = (1, 2, 5)
TOL = to.TOL
INT32_MAX = 2 ** 31 - 1
W = _lib.GGNN_LABEL_STATUS_WORDS

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def to_dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the oracles, frame by frame: computed once, shared, left unchanged ------------------------------------------------------

def restated_frames(key, frames_kw, **common):
    """labelcheck.label on every frame's keywords -> the list of its results."""
    return cached(("label", key), lambda: [lc.label(**dict(kw, **common)) for kw in frames_kw])


def restated_quat_frames(key, quats, **common):
    return cached(("orient", key), lambda: [oc.label(q, **common) for q in quats])


def voronoi_frames(shape, boundary, T=5):
    """test_label's voronoi_map, a seed a frame: the frames differ in their cells, their noise and their n_grains."""
    maps = [tl.voronoi_map(*shape, boundary, 11 + t) for t in range(T)]
    return np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])


def quat_frames(shape, boundary, T=5):
    return np.stack([to.noisy_recipe(shape, boundary, 5 + t) for t in range(T)])


def assert_stack(got, want, what, means_key="mean_angles"):
    """(images, n_grains, means [T, K, capacity] or None, statuses) of a stacked call against per-frame results."""
    images, n_grains, means, statuses = got
    T = len(want)
    assert images.dtype == torch.int32 and images.shape[0] == T and len(n_grains) == T == len(statuses), what
    host = images.cpu().numpy()
    for t, r in enumerate(want):
        assert statuses[t] == r["status"], (what, t, statuses[t], r["status"])
        assert statuses[t]["n_bound_hits"] == 0 and n_grains[t] == r["n_grain"], (what, t)
        assert np.array_equal(host[t], r["image"]), (what, t)
    if want[0].get(means_key) is None:
        assert means is None, what
        return
    assert means.dtype == torch.float32 and means.shape[0] == T, what
    m = means.cpu().numpy()
    for t, r in enumerate(want):
        n = r[means_key].shape[1]
        assert np.array_equal(m[t, :, :n].view(np.uint32), r[means_key].view(np.uint32)), (what, t)
        assert not m[t, :, n:].any(), (what, t)                      # rows beyond a frame's grains are zero


def run_maps(**kw):
    return vz.label_maps(**{k: (to_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()})


def run_quat_maps(quats, tol, **kw):
    return vz.label_orientation_maps(to_dev(quats), tol, **{k: (to_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()})


# ---- CPU: the ABI ----------------------------------------------------------------------------------------------------------------

def struct_fields(src, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    return re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_header_binding_and_struct_sizes_agree():
    src = open(os.path.join(ROOT, "include", "ggnn.h")).read()
    assert struct_fields(src, "ggnn_label_stack_args") == [f[0] for f in _lib.LabelStackArgs._fields_]
    assert struct_fields(src, "ggnn_label_orient_stack_args") == [f[0] for f in _lib.LabelOrientStackArgs._fields_]
    # the single call's fields plus T
    assert [f for f in struct_fields(src, "ggnn_label_stack_args") if f != "T"] == struct_fields(src, "ggnn_label_args")
    assert [f for f in struct_fields(src, "ggnn_label_orient_stack_args") if f != "T"] == struct_fields(src, "ggnn_label_orient_args")
    assert ctypes.sizeof(_lib.LabelStackArgs) == ctypes.sizeof(_lib.LabelArgs) + 8 == 8 * 8 + 5 * 8 + 4 * 4
    assert ctypes.sizeof(_lib.LabelOrientStackArgs) == ctypes.sizeof(_lib.LabelOrientArgs) + 8 == 7 * 8 + 5 * 8 + 4 * 4
    assert {"ggnn_label_grains_stack", "ggnn_label_stack_workspace_bytes", "ggnn_label_orientations_stack",
            "ggnn_label_orient_stack_workspace_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    assert _lib.load().ggnn_version() == 26 == _lib.GGNN_ABI_VERSION
    assert "frame t's image, means and nine words are ggnn_label_grains'" in src


def test_workspace_queries():
    lib = _lib.load()
    for nx, ny in ((3, 3), (65, 15), (64, 16), (127, 33), (501, 501), (4096, 4096)):
        for K in range(5):
            assert lib.ggnn_label_stack_workspace_bytes(1, nx, ny, K) == lib.ggnn_label_workspace_bytes(nx, ny, K) > 0
        assert lib.ggnn_label_orient_stack_workspace_bytes(1, nx, ny) == lib.ggnn_label_orient_workspace_bytes(nx, ny) > 0
        assert lib.ggnn_label_orient_stack_workspace_bytes(3, nx, ny) == lib.ggnn_label_stack_workspace_bytes(3, nx, ny, 4)
    # the per-frame carve times T: every per-pixel array of T N entries, every per-chunk array of T ceil(N / 1024)
    one, seven = lib.ggnn_label_stack_workspace_bytes(1, 501, 501, 2), lib.ggnn_label_stack_workspace_bytes(7, 501, 501, 2)
    assert 7 * 501 * 501 * (21 + 16) <= seven <= 7 * one + 8 * 4352
    # refused: sizes the single call refuses, T < 1, more than INT32_MAX pixels
    for T, nx, ny, K in ((0, 8, 8, 0), (-1, 8, 8, 0), (2, 2, 8, 0), (2, 8, 2, 0), (2, 1 << 15, 8, 0), (2, 8, 8, 5), (2, 8, 8, -1),
                         (3, 32767, 32767, 0), (INT32_MAX // 9 + 1, 3, 3, 0), (1 << 40, 3, 3, 0), (1 << 62, 1000, 1000, 0)):
        assert lib.ggnn_label_stack_workspace_bytes(T, nx, ny, K) == 0, (T, nx, ny, K)
        if 0 <= K <= 4:
            assert lib.ggnn_label_orient_stack_workspace_bytes(T, nx, ny) == 0, (T, nx, ny)
    assert lib.ggnn_label_stack_workspace_bytes(INT32_MAX // 9, 3, 3, 0) > 0            # T nx ny <= INT32_MAX is taken
    assert lib.ggnn_label_stack_workspace_bytes(2, 32767, 32767, 0) > 0


def test_grains_entry_point_validates_on_the_host():
    lib = _lib.load()
    assert lib.ggnn_label_grains_stack(None, None) == -1
    need = lib.ggnn_label_stack_workspace_bytes(3, 32, 32, 2)
    buf = (ctypes.c_int64 * 64)()                 # (host memory: refused before anything would be launched)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(**kw):
        A = _lib.LabelStackArgs(None, p, None, p, p, p, p, need, 3, 32, 32, 64, 1, 0.001, 2, 4, 0)
        A.image = None                            # (so that a call that passes every other check still launches nothing)
        for k, v in kw.items():
            setattr(A, k, v)
        return lib.ggnn_label_grains_stack(ctypes.byref(A), None)
    assert call() == -1
    single = (dict(ids=p), dict(angles=None), dict(status=None), dict(workspace=None), dict(mean_angles=None), dict(nx=2), dict(ny=2),
              dict(nx=1 << 15), dict(K=0), dict(K=5), dict(tol=-1.0), dict(tol=float("nan")), dict(min_pixels=0), dict(max_sweeps=-1),
              dict(max_sweeps=_lib.GGNN_LABEL_MAX_SWEEPS + 1), dict(grain_capacity=0), dict(grain_capacity=2 ** 31 - 1),
              dict(boundary=2), dict(status=p.value + 4), dict(workspace=p.value + 4), dict(mean_angles=p.value + 2),
              dict(workspace_bytes=need - 1), dict(angles=None, ids=p, K=2))
    stack = (dict(T=0), dict(T=-1), dict(T=4), dict(T=INT32_MAX // 1024 + 1, workspace_bytes=1 << 62), dict(T=1 << 40, workspace_bytes=1 << 62),
             dict(T=3, nx=32767, ny=32767, workspace_bytes=1 << 62))
    for bad in single + stack:
        assert call(image=p, **bad) == -1, bad


def test_orientations_entry_point_validates_on_the_host():
    lib = _lib.load()
    assert lib.ggnn_label_orientations_stack(None, None) == -1
    need = lib.ggnn_label_orient_stack_workspace_bytes(3, 32, 32)
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    c = float(oc.cos_half(0.03))

    def call(**kw):
        A = _lib.LabelOrientStackArgs(p, None, p, p, p, p, need, 3, 32, 32, 64, 1, c, _lib.GGNN_SYM_CUBIC, 4, 0)
        A.image = None
        for k, v in kw.items():
            setattr(A, k, v)
        return lib.ggnn_label_orientations_stack(ctypes.byref(A), None)
    assert call() == -1
    single = (dict(quats=None), dict(mean_quats=None), dict(status=None), dict(workspace=None), dict(nx=2), dict(ny=2), dict(nx=1 << 15),
              dict(ny=1 << 15), dict(cos_half_tol=float(oc.cos_half(np.pi / 2))), dict(cos_half_tol=0.5), dict(cos_half_tol=1.0000001),
              dict(cos_half_tol=float("nan")), dict(cos_half_tol=-0.9), dict(symmetry=2), dict(symmetry=-1), dict(boundary=2),
              dict(min_pixels=0), dict(max_sweeps=-1), dict(max_sweeps=_lib.GGNN_LABEL_MAX_SWEEPS + 1), dict(grain_capacity=0),
              dict(grain_capacity=2 ** 31 - 1), dict(status=p.value + 4), dict(workspace=p.value + 4), dict(mean_quats=p.value + 2),
              dict(quats=p.value + 2), dict(workspace_bytes=need - 1), dict(image=p.value + 2))
    stack = (dict(T=0), dict(T=-1), dict(T=4), dict(T=INT32_MAX // 1024 + 1, workspace_bytes=1 << 62), dict(T=1 << 40, workspace_bytes=1 << 62))
    for bad in single + stack:
        assert call(**dict(dict(image=p), **bad)) == -1, bad


def test_python_entry_points_refuse_what_they_cannot_take():
    host = torch.ones(2, 8, 8, dtype=torch.int32)
    quats = torch.zeros(2, 4, 8, 8)
    for kw, match in ((dict(), "exactly one"), (dict(ids=host, angles=host), "exactly one"), (dict(ids=host), "device"),
                      (dict(ids=host, boundary="open"), "boundary")):
        with pytest.raises(_lib.GGNNError, match=match):
            vz.label_maps(**kw)
    with pytest.raises(_lib.GGNNError, match=r"\[T, 4, ny, nx\]"):
        vz.label_orientation_maps(quats, 0.03)                       # a host tensor
    for bad in (dict(tol=None), dict(tol=2.0), dict(symmetry="hexagonal"), dict(boundary="open")):
        with pytest.raises(_lib.GGNNError):
            vz.label_orientation_maps(quats, **dict(dict(tol=0.03), **bad))
    with pytest.raises(_lib.GGNNError, match="equal-shaped"):
        vz.samples_from_orientation_maps(host, host[:1], 2.0, 0.4, 1e-3)
    with pytest.raises(_lib.GGNNError, match="equal-shaped"):
        vz.samples_from_orientation_maps(host[0], host[0], 2.0, 0.4, 1e-3)    # one map is no stack
    with pytest.raises(_lib.GGNNError, match="equal-shaped"):
        vz.samples_from_euler_maps(torch.zeros(2, 8, 8), torch.zeros(2, 8, 8), torch.zeros(2, 8, 7), 2.0, 0.4, 0.03)


@pytest.mark.gpu
def test_python_entry_points_refuse_wrong_ranks_dtypes_and_masks():
    ids = torch.ones(2, 8, 8, dtype=torch.int32, device=DEV)
    angles = torch.zeros(2, 2, 8, 8, device=DEV)
    quats = torch.zeros(2, 4, 8, 8, device=DEV)
    quats[:, 0] = 1
    cases = ((dict(ids=ids[0]), "integer"), (dict(ids=ids.float()), "integer"), (dict(ids=ids[:, :2]), "3 x 3"),
             (dict(angles=angles), "tol"), (dict(angles=angles[0], tol=0.1), "float32"), (dict(angles=angles.double(), tol=0.1), "float32"),
             (dict(angles=torch.zeros(2, 5, 8, 8, device=DEV), tol=0.1), "K <= 4"), (dict(ids=ids[:0]), "at least one map"),
             (dict(ids=ids, valid=torch.ones(8, 8, device=DEV)), "mask"), (dict(ids=ids, valid=torch.ones(2, 8, 8)), "mask"),
             (dict(ids=ids, min_pixels=0), "min_pixels"), (dict(ids=ids, max_sweeps=-1), "max_sweeps"), (dict(ids=ids, grain_capacity=0), "grain_capacity"))
    for kw, match in cases:
        with pytest.raises(_lib.GGNNError, match=match):
            vz.label_maps(**kw)
    for kw in (dict(quats=quats[0]), dict(quats=quats[:, :3]), dict(quats=quats.double()), dict(quats=quats[:0]), dict(quats=quats[..., :2]),
               dict(quats=quats, valid=torch.ones(8, 8, device=DEV)), dict(quats=quats, valid=torch.ones(2, 8, 8)), dict(quats=quats, min_pixels=0)):
        with pytest.raises(_lib.GGNNError):
            vz.label_orientation_maps(tol=0.03, **kw)


# ---- GPU: Voronoi stacks with 1 % noise against the restatements ---------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_voronoi_stacks_equal_the_restatement_frame_by_frame(shape, boundary):
    ids, angles = voronoi_frames(shape, boundary)
    for mp in (1, 3):
        for mode in ("ids", "angles"):
            frames_kw = [dict(ids=i) for i in ids] if mode == "ids" else [dict(angles=a, tol=1e-3) for a in angles]
            want = restated_frames(("voronoi", shape, boundary, mode, mp), frames_kw, min_pixels=mp, boundary=boundary)
            if shape != (3, 3) and mp == 1:
                assert len({r["n_grain"] for r in want}) > 1                    # (the frames do differ in their number of grains)
            for T in DEPTHS:
                kw = dict(ids=ids[:T]) if mode == "ids" else dict(angles=angles[:T], tol=1e-3)
                assert_stack(run_maps(min_pixels=mp, boundary=boundary, **kw), want[:T], (shape, boundary, mode, mp, T))


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_quaternion_stacks_equal_the_restatement_frame_by_frame(shape, boundary):
    quats = quat_frames(shape, boundary)
    for symmetry in ("cubic", "none"):
        for mp in (1, 3):
            want = restated_quat_frames((shape, boundary, symmetry, mp), quats, tol=TOL, min_pixels=mp, boundary=boundary, symmetry=symmetry)
            for T in DEPTHS:
                got = run_quat_maps(quats[:T], TOL, min_pixels=mp, boundary=boundary, symmetry=symmetry)
                assert_stack(got, want[:T], (shape, boundary, symmetry, mp, T), "mean_quats")


# ---- frames do not leak ----------------------------------------------------------------------------------------------------------

def chained_frames(shape, boundary, T=4):
    """Frame t's bottom row equals frame t + 1's top row in ids, while its own top row differs from its bottom row: a stack
    read as one taller image, or a wrap that lands in the neighbouring frame, would link them."""
    ids, _ = voronoi_frames(shape, boundary, T)
    ids = ids.copy()
    for t in range(T):
        ids[t, 0], ids[t, -1] = 1000 + t, 1001 + t
    assert all(np.array_equal(ids[t, -1], ids[t + 1, 0]) and not np.array_equal(ids[t, 0], ids[t, -1]) for t in range(T - 1))
    return ids


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_frames_do_not_leak(boundary):
    shape = (15, 65)
    ids = chained_frames(shape, boundary)
    angles = np.stack([ids * 0.001, ids * 0.002], 1).astype(np.float32)                     # the same chain in two angle channels
    angles[np.broadcast_to((ids == 0)[:, None], angles.shape)] = np.nan
    want = restated_frames(("chained", boundary), [dict(ids=i) for i in ids], boundary=boundary, min_pixels=2)
    for kw in (dict(ids=ids), dict(angles=angles, tol=1e-4)):
        forward = run_maps(boundary=boundary, min_pixels=2, **kw)
        backward = run_maps(boundary=boundary, min_pixels=2, **{k: (np.ascontiguousarray(v[::-1]) if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
        assert torch.equal(forward[0].flip(0), backward[0]) and forward[1][::-1] == backward[1] and forward[3][::-1] == backward[3]
        if forward[2] is not None:
            assert torch.equal(forward[2].flip(0), backward[2])
        if "ids" in kw:
            assert_stack(forward, want, ("chained", boundary))
        else:
            assert forward[3] == [r["status"] for r in want] and np.array_equal(forward[0].cpu().numpy(), np.stack([r["image"] for r in want]))
    # five copies of one frame: five identical results, each the single call's
    one = to_dev(ids[1])
    image, n_grain, _, status = vz.label_grains(ids=one, boundary=boundary, min_pixels=2)
    images, n_grains, _, statuses = vz.label_maps(ids=one[None].repeat(5, 1, 1), boundary=boundary, min_pixels=2)
    assert n_grains == [n_grain] * 5 and statuses == [status] * 5 and all(torch.equal(images[t], image) for t in range(5))
    q = to_dev(quat_frames(shape, boundary, 2)[1])
    image, n_grain, means, status = vz.label_orientations(q, TOL, boundary=boundary, min_pixels=2)
    images, n_grains, all_means, statuses = vz.label_orientation_maps(q[None].repeat(5, 1, 1, 1), TOL, boundary=boundary, min_pixels=2)
    assert n_grains == [n_grain] * 5 and statuses == [status] * 5
    for t in range(5):
        assert torch.equal(images[t], image) and torch.equal(all_means[t, :, :n_grain].view(torch.int32), means.view(torch.int32)), t


# ---- counters per frame where several frames share a wave --------------------------------------------------------------------------

def nine_small_frames():
    """Nine 3 x 3 frames (81 pixels: two waves, the first holds seven frames and a part of the eighth) whose status rows differ
    from neighbour to neighbour, with min_pixels = 2."""
    rows = tl.rows
    clean, empty = np.full((3, 3), 4, np.int32), np.zeros((3, 3), np.int32)
    grains = rows([1, 1, 2], [3, 3, 2], [3, 3, 2])                    # components of two pixels and more
    specks = np.arange(1, 10, dtype=np.int32).reshape(3, 3)          # nine components of one pixel: all specks, all unfilled
    mixed = rows([1, 1, 1], [1, 5, 1], [1, 1, 0])                     # a grain, a speck and a non-indexed pixel: a sweep runs
    holes = rows([2, 0, 2], [0, 2, 0], [2, 0, 2])                     # five one-pixel components (fewer through the wrap) and four holes
    return np.stack([clean, empty, grains, specks, empty, mixed, clean, holes, grains[::-1].copy()])


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_counters_land_in_their_own_frame_at_3x3(boundary):
    ids = nine_small_frames()
    want = restated_frames(("nine", boundary), [dict(ids=i) for i in ids], boundary=boundary, min_pixels=2)
    rows_ = [r["status"] for r in want]
    assert all(a != b for a, b in zip(rows_, rows_[1:]))
    assert rows_[1]["n_grains"] == 0 and rows_[1]["n_unfilled"] == 9 == rows_[1]["n_invalid_in"] and want[1]["n_grain"] == (boundary == "noflux")
    assert rows_[3]["n_specks"] == 9 == rows_[3]["n_speck_pixels"] and rows_[0]["n_components"] == 1 and rows_[5]["n_sweeps"] == 1
    for word in ("n_components", "n_specks", "n_speck_pixels", "n_invalid_in", "n_grains", "n_sweeps", "n_unfilled"):
        assert len({r[word] for r in rows_}) > 1, word                  # every counter takes more than one value across the stack
    assert_stack(run_maps(ids=ids, boundary=boundary, min_pixels=2), want, ("nine", boundary))
    angles = ids[:, None].astype(np.float32) * np.float32(0.5)
    angles[angles == 0] = np.nan
    got = run_maps(angles=angles, tol=0.1, boundary=boundary, min_pixels=2)
    assert got[3] == rows_ and np.array_equal(got[0].cpu().numpy(), np.stack([r["image"] for r in want]))
    # the same frames as orientations: an id an orientation, 0 not indexed
    table = oc.recipe(3, 3, "periodic", 3, n_cells=12)["cell_quats"].astype(np.float32)        # (more than 5 degrees apart)
    quats = np.ascontiguousarray(table[:, np.maximum(ids, 1)].transpose(1, 0, 2, 3))
    quats[np.broadcast_to((ids == 0)[:, None], quats.shape)] = np.nan
    got = run_quat_maps(quats, TOL, boundary=boundary, min_pixels=2)
    assert got[3] == rows_ and np.array_equal(got[0].cpu().numpy(), np.stack([r["image"] for r in want]))


# ---- sweeps per frame ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_sweeps_are_counted_and_stopped_per_frame():
    ones = np.ones((7, 7), np.int32)
    one_hole, block = ones.copy(), ones.copy()
    one_hole[3, 3] = 0
    block[2:5, 2:5] = 0
    ids = np.stack([ones, one_hole, block, np.zeros((7, 7), np.int32), block, ones])
    for max_sweeps, sweeps, unfilled in ((64, [0, 1, 2, 0, 2, 0], [0, 0, 0, 49, 0, 0]), (1, [0, 1, 1, 0, 1, 0], [0, 0, 1, 49, 1, 0]),
                                         (0, [0] * 6, [0, 1, 9, 49, 9, 0])):
        want = restated_frames(("sweeps", max_sweeps), [dict(ids=i) for i in ids], max_sweeps=max_sweeps)
        assert [r["status"]["n_sweeps"] for r in want] == sweeps and [r["status"]["n_unfilled"] for r in want] == unfilled
        got = run_maps(ids=ids, max_sweeps=max_sweeps)
        assert_stack(got, want, ("sweeps", max_sweeps))
        assert [s["n_sweeps"] for s in got[3]] == sweeps and [s["n_unfilled"] for s in got[3]] == unfilled
        if max_sweeps == 1:                                           # the hole's centre stays open in its own frames alone
            assert got[0][2, 3, 3] == 0 == got[0][4, 3, 3] and int((got[0] == 0).sum()) == 2 + 49


# ---- union-find stress inside a stack ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_union_find_stress_inside_a_stack(boundary):
    ny, nx = 2 * tl.TY + 1, 3 * tl.TX + 1
    assert (ny, nx) == (33, 193)
    ids = np.stack([tl.serpentine(ny, nx), tl.comb(ny, nx), tl.spiral(ny, nx), tl.serpentine(ny, nx, True)])
    want = restated_frames(("stress", boundary), [dict(ids=i) for i in ids], boundary=boundary, max_sweeps=0)
    assert [r["status"]["n_components"] for r in want] == [1, 1, 1 if boundary == "periodic" else 2, 1]
    got = run_maps(ids=ids, boundary=boundary, max_sweeps=0)
    assert [s["n_bound_hits"] for s in got[3]] == [0] * 4
    assert_stack(got, want, ("stress", boundary))
    quats = np.stack([oc.recipe(ny, nx, "periodic", 8 + t, seeds=[(0.0, 0.0)])["quats"] for t in range(3)])
    quats[np.broadcast_to((ids[:3] == 0)[:, None], quats.shape)] = np.nan
    want = restated_quat_frames(("stress", boundary), quats, tol=TOL, boundary=boundary, max_sweeps=0)
    assert_stack(run_quat_maps(quats, TOL, boundary=boundary, max_sweeps=0), want, ("stress quats", boundary), "mean_quats")


# ---- a capacity that ends inside one frame's grains ----------------------------------------------------------------------------------

def frames_with_the_most_grains_in_the_middle(counts):
    """Indices (a, b, c) of three frames with counts[b] > counts[a], counts[c]."""
    b = int(np.argmax(counts))
    rest = [i for i in range(len(counts)) if counts[i] < counts[b]]
    assert len(rest) >= 2
    return rest[0], b, rest[1]


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_a_capacity_inside_one_frames_grains(boundary):
    shape = (33, 127)
    ids, angles = voronoi_frames(shape, boundary)
    full = restated_frames(("voronoi", shape, boundary, "angles", 1), [dict(angles=a, tol=1e-3) for a in angles], min_pixels=1, boundary=boundary)
    pick = list(frames_with_the_most_grains_in_the_middle([r["n_grain"] for r in full]))
    cap = full[pick[1]]["n_grain"] - 1
    assert full[pick[0]]["n_grain"] <= cap >= full[pick[2]]["n_grain"]
    want = restated_frames(("capacity", boundary), [dict(angles=angles[t], tol=1e-3) for t in pick], boundary=boundary, grain_capacity=cap)
    assert [r["status"]["overflow"] for r in want] == [0, 1, 0]
    got = run_maps(angles=angles[pick], tol=1e-3, boundary=boundary, grain_capacity=cap)
    assert got[2].shape == (3, 2, cap) and [s["overflow"] for s in got[3]] == [0, 1, 0]
    assert_stack(got, want, ("capacity", boundary))
    assert np.array_equal(got[0].cpu().numpy(), np.stack([full[t]["image"] for t in pick]))     # every image is complete
    quats = quat_frames(shape, boundary)
    full = restated_quat_frames((shape, boundary, "cubic", 1), quats, tol=TOL, min_pixels=1, boundary=boundary, symmetry="cubic")
    pick = list(frames_with_the_most_grains_in_the_middle([r["n_grain"] for r in full]))
    cap = full[pick[1]]["n_grain"] - 1
    want = restated_quat_frames(("capacity", boundary), quats[pick], tol=TOL, boundary=boundary, grain_capacity=cap)
    got = run_quat_maps(quats[pick], TOL, boundary=boundary, grain_capacity=cap)
    assert [s["overflow"] for s in got[3]] == [0, 1, 0]
    assert_stack(got, want, ("capacity quats", boundary), "mean_quats")


# ---- guards ----------------------------------------------------------------------------------------------------------------------------

GUARD = 64


def guarded(T, ny, nx, K, cap, need, call):
    """Canaries before and after the images, the means, the status and the workspace; call(image, means, status, ws) launches."""
    image = torch.full((T * ny * nx + 2 * GUARD,), -7, dtype=torch.int32, device=DEV)
    means = torch.full((T * max(K, 1) * cap + 2 * GUARD,), -7.0, dtype=torch.float32, device=DEV)
    status = torch.full((T * W + 2 * GUARD,), -7, dtype=torch.int64, device=DEV)
    ws = torch.full((need + 2 * 256,), 0x5A, dtype=torch.uint8, device=DEV)
    call(image[GUARD:].data_ptr(), means[GUARD:].data_ptr(), status[GUARD:].data_ptr(), ws[256:].data_ptr())
    torch.cuda.synchronize()
    assert bool((ws[:256] == 0x5A).all()) and bool((ws[256 + need:] == 0x5A).all())
    assert bool((status[:GUARD] == -7).all()) and bool((status[GUARD + T * W:] == -7).all())
    assert bool((image[:GUARD] == -7).all()) and bool((image[GUARD + T * ny * nx:] == -7).all())
    assert bool((means[:GUARD] == -7).all()) and bool((means[GUARD + T * max(K, 1) * cap:] == -7).all())
    return (image[GUARD:GUARD + T * ny * nx].view(T, ny, nx), means[GUARD:GUARD + T * max(K, 1) * cap].view(T, max(K, 1), cap),
            status[GUARD:GUARD + T * W].view(T, W))


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_guarded_arrays_of_both_entry_points(boundary):
    lib = _lib.load()
    T, (ny, nx) = 3, (15, 65)
    ids, angles = voronoi_frames((ny, nx), boundary, T)
    mask = np.ones((T, ny, nx), np.uint8)
    mask[1, 3:6, 30:40] = 0
    d_mask = to_dev(mask)
    for mode in ("ids", "angles"):
        frames_kw = [dict(ids=ids[t], valid=mask[t]) if mode == "ids" else dict(angles=angles[t], tol=1e-3, valid=mask[t]) for t in range(T)]
        full = [lc.label(min_pixels=3, boundary=boundary, **kw) for kw in frames_kw]
        cap = max(r["n_grain"] for r in full) - 1                       # at least one frame overflows
        want = [lc.label(min_pixels=3, boundary=boundary, grain_capacity=cap, **kw) for kw in frames_kw]
        K = 0 if mode == "ids" else 2
        need = lib.ggnn_label_stack_workspace_bytes(T, nx, ny, K)
        d_in = to_dev(ids) if mode == "ids" else to_dev(angles)

        def call(image, means, status, ws):
            A = _lib.LabelStackArgs(_lib.ptr(d_in) if K == 0 else None, _lib.ptr(d_in) if K else None, _lib.ptr(d_mask), image, means if K else None,
                                    status, ws, need, T, nx, ny, cap, 3, float(np.float32(1e-3)) if K else 0.0, K, 64, vz.BOUNDARIES[boundary])
            _lib.check(lib.ggnn_label_grains_stack(ctypes.byref(A), _lib.current_stream()), "ggnn_label_grains_stack")
        image, means, status = guarded(T, ny, nx, K, cap, need, call)
        assert any(r["status"]["overflow"] for r in want)
        for t, r in enumerate(want):
            assert dict(zip(lc.STATUS, status[t].tolist())) == r["status"] and np.array_equal(image[t].cpu().numpy(), r["image"]), (mode, t)
            if K == 0:
                continue
            n = r["mean_angles"].shape[1]
            assert np.array_equal(means[t, :, :n].cpu().numpy().view(np.uint32), r["mean_angles"].view(np.uint32)), (mode, t)
            assert bool((means[t, :, n:] == -7).all()), (mode, t)       # rows from a frame's n_grain on are not written
        if K == 0:
            assert bool((means == -7).all())
    quats = quat_frames((ny, nx), boundary, T)
    full = [oc.label(quats[t], TOL, valid=mask[t], min_pixels=3, boundary=boundary) for t in range(T)]
    cap = max(r["n_grain"] for r in full) - 1
    want = [oc.label(quats[t], TOL, valid=mask[t], min_pixels=3, boundary=boundary, grain_capacity=cap) for t in range(T)]
    need = lib.ggnn_label_orient_stack_workspace_bytes(T, nx, ny)
    d_q = to_dev(quats)

    def call_quats(image, means, status, ws):
        A = _lib.LabelOrientStackArgs(_lib.ptr(d_q), _lib.ptr(d_mask), image, means, status, ws, need, T, nx, ny, cap, 3, float(oc.cos_half(TOL)),
                                      _lib.GGNN_SYM_CUBIC, 64, vz.BOUNDARIES[boundary])
        _lib.check(lib.ggnn_label_orientations_stack(ctypes.byref(A), _lib.current_stream()), "ggnn_label_orientations_stack")
    image, means, status = guarded(T, ny, nx, 4, cap, need, call_quats)
    for t, r in enumerate(want):
        assert dict(zip(lc.STATUS, status[t].tolist())) == r["status"] and np.array_equal(image[t].cpu().numpy(), r["image"]), t
        n = r["mean_quats"].shape[1]
        assert np.array_equal(means[t, :, :n].cpu().numpy().view(np.uint32), r["mean_quats"].view(np.uint32)), t
        assert bool((means[t, :, n:] == -7).all()), t


# ---- replays ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_two_runs_and_a_captured_graph_give_the_same_bits():
    shape = (33, 127)
    _, angles = voronoi_frames(shape, "periodic")
    want = restated_frames(("voronoi", shape, "periodic", "angles", 3), [dict(angles=a, tol=1e-3) for a in angles], min_pixels=3, boundary="periodic")
    quats = quat_frames(shape, "periodic")
    want_q = restated_quat_frames((shape, "periodic", "cubic", 3), quats, tol=TOL, min_pixels=3, boundary="periodic", symmetry="cubic")
    for f, args, wanted in ((vz._label_stack, (None, to_dev(angles), 1e-3, None, 3, 64, "periodic", None), want),
                            (vz._label_orient_stack, (to_dev(quats), TOL, None, 3, 64, "periodic", None, "cubic"), want_q)):
        first, second = f(*args), f(*args)                              # (also the warm-up of the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            held = f(*args)
        graph.replay()                                                  # (a replay starts from its own zeroed words and sums)
        torch.cuda.synchronize()
        once = {k: held[k].clone() for k in ("image", "means", "status")}
        graph.replay()
        torch.cuda.synchronize()
        for k in ("image", "means", "status"):
            assert torch.equal(first[k], second[k]) and torch.equal(first[k], once[k]) and torch.equal(first[k], held[k]), k
        assert held["status"].tolist() == [[r["status"][w] for w in lc.STATUS] for r in wanted]
        assert np.array_equal(held["image"].cpu().numpy(), np.stack([r["image"] for r in wanted]))


# ---- the recorded sequence: the stack against seven single calls of the device -------------------------------------------------------

@pytest.mark.gpu
def test_the_recorded_sequence_equals_seven_single_calls():
    g = tl.golden()
    frames = g["frames"]
    assert frames.shape == (7, 501, 501)
    ids = to_dev(frames)
    images, n_grains, means, statuses = vz.label_maps(ids=ids)
    assert means is None
    for t in range(7):
        image, n_grain, _, status = vz.label_grains(ids=ids[t])
        assert torch.equal(images[t], image) and n_grains[t] == n_grain and statuses[t] == status, t
    noisy = np.stack([lc.noisy(frames[t], g["theta"], 0.04, t)[1] for t in range(7)])
    dev = to_dev(noisy)
    for boundary in BOUNDARIES:
        images, n_grains, means, statuses = vz.label_maps(angles=dev, tol=1e-3, min_pixels=8, boundary=boundary)
        assert max(s["n_sweeps"] for s in statuses) >= 1 and len({tuple(s.values()) for s in statuses}) > 1
        for t in range(7):
            image, n_grain, mean, status = vz.label_grains(angles=dev[t], tol=1e-3, min_pixels=8, boundary=boundary)
            assert torch.equal(images[t], image) and n_grains[t] == n_grain and statuses[t] == status, (boundary, t)
            assert torch.equal(means[t, :, :n_grain].view(torch.int32), mean.view(torch.int32)) and not bool(means[t, :, n_grain:].any()), (boundary, t)


# ---- the sequences: one stacked labelling call, one link call, one read-back --------------------------------------------------------

def entries_of(monkeypatch):
    """Collects the entry names that pass through _lib.check."""
    names, check = [], _lib.check

    def collecting(code, name, *a, **kw):
        names.append(name)
        return check(code, name, *a, **kw)
    monkeypatch.setattr(_lib, "check", collecting)
    return names


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_label_sequence_makes_one_stacked_call(boundary, monkeypatch):
    shape, T = (33, 127), 5
    ids, angles = voronoi_frames(shape, boundary, T)
    want = restated_frames(("voronoi", shape, boundary, "angles", 3), [dict(angles=a, tol=1e-3) for a in angles], min_pixels=3, boundary=boundary)
    dev = to_dev(angles)
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        names, counted = entries_of(m), to.Counted(m)
        frames, n_grain, theta, report = vz.label_sequence(angles=dev, tol=1e-3, min_pixels=3, boundary=boundary)
        assert counted.n == 1                                           # one read-back
    assert names.count("ggnn_label_grains_stack") == 1 and names.count("ggnn_link_labels") == 1
    assert "ggnn_label_grains" not in names and "ggnn_label_orientations" not in names
    assert report["label"] == [r["status"] for r in want] and frames.shape == (T, *shape)
    assert lc.same_partition(frames[0].cpu().numpy(), want[0]["image"])


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_label_orientation_sequence_makes_one_stacked_call(boundary, monkeypatch):
    shape, T = (33, 127), 5
    d = to.drifting_frames(shape, boundary, T)
    want = restated_quat_frames(("drifting", boundary), d["quats"], tol=TOL, boundary=boundary, grain_capacity=300)
    quats = to_dev(d["quats"])
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        names, counted = entries_of(m), to.Counted(m)
        frames, n_grain, quat, report = vz.label_orientation_sequence(quats, TOL, boundary=boundary, grain_capacity=300)
        assert counted.n == 1
    assert names.count("ggnn_label_orientations_stack") == 1 and names.count("ggnn_link_labels") == 1
    assert "ggnn_label_grains" not in names and "ggnn_label_orientations" not in names and "ggnn_label_grains_stack" not in names
    host = frames.cpu().numpy()
    assert report["label"] == [r["status"] for r in want] and all(lc.same_partition(host[t], d["cells"][t]) for t in range(T))
    n0 = want[0]["n_grain"]                                             # frame 0 keeps its ids: the first rows are its means
    assert np.array_equal(quat[:, :n0].cpu().numpy().view(np.uint32), want[0]["mean_quats"].view(np.uint32))


# ---- ensembles of maps into one union rollout -----------------------------------------------------------------------------------------

def assert_member_equals(union, t, own):
    """Trajectory t cut from the union (x, ei, ea, offsets) against a single map's (x, ei, ea), bit for bit."""
    X, EI, EA, off = union
    x, ei, ea = own
    og, oj = off["grain"], off["joint"]
    for k, o in (("grain", og), ("joint", oj)):
        assert x[k].dtype == X[k].dtype and torch.equal(X[k][o[t]:o[t + 1]], x[k]), (t, k)
    for et in EDGE_TYPES:
        shift = torch.tensor([[off[et[0]][t]], [off[et[2]][t]]], device=DEV)
        assert torch.equal(EI[et][:, 3 * oj[t]:3 * oj[t + 1]] - shift, ei[et]), (t, et)
        assert torch.equal(EA[et][3 * oj[t]:3 * oj[t + 1]], ea[et]), (t, et)


def five_union_steps(X, EI, EA, off, boundary, shape, grid):
    from graingraphnn_amd import GrainRollout
    kw = dict(boundary="noflux", max_y=vz.image_max_y(shape[1], shape[0], grid), traj_offsets=off) if boundary == "noflux" else {}
    Rm, Cm = product_models(10020, 1.0, DEV)
    ro = GrainRollout(Rm, Cm, X, EI, EA, 6, refresh_centres=True, **kw)
    for _ in range(5):
        pred = ro.step()
        assert all(bool(torch.isfinite(v).all()) for v in pred.values())
    assert not ro.range_exceeded()


G3, R3 = [2.0, 3.5, 1.2], [0.4, 0.9, 0.25]


def orientation_maps(boundary):
    """Three measured maps of one shape -> (angles float32 [3, 2, ny, nx], tol, min_pixels): periodic, frame 0 of the recorded run
    under the three noise recipes of test_label; no-flux, the recorded no-flux structure with three draws of per-grain angles."""
    if boundary == "periodic":
        return np.stack([tl.golden_inputs(tag)[1] for tag in sorted(tl.NOISE)]), 1e-3, 8
    field = np.load(os.path.join(GOLDEN, "grain_image_cfg1.npz"))["noflux__alpha_field"].astype(np.int32)
    maps = []
    for seed in (7, 8, 9):
        rs = np.random.RandomState(seed)
        maps.append(tl.f32(np.stack([rs.uniform(0, np.pi / 2, 102), rs.uniform(0, np.pi / 2, 102)]))[:, field])
    return np.stack(maps), 1e-4, 1


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
@torch.no_grad()
def test_samples_from_orientation_maps(boundary, monkeypatch):
    angles, tol, mp = cached(("orientation maps", boundary), lambda: orientation_maps(boundary))
    dev = to_dev(angles)
    kw = dict(span=6, patch_pixels=501 ** 2, grid="points", boundary=boundary)
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        counted = to.Counted(m)
        X, EI, EA, off, images, statuses = vz.samples_from_orientation_maps(dev[:, 0], dev[:, 1], G3, R3, tol, min_pixels=mp, **kw)
        assert counted.n == 3                                           # the label status, the means, the vectoriser's status
    assert images.shape == (3, 501, 501) and len(statuses) == 3 and len(off["grain"]) == 4
    for t in range(3):
        x, ei, ea, image, status = vz.sample_from_orientations(dev[t, 0], dev[t, 1], G3[t], R3[t], tol, min_pixels=mp, **kw)
        assert torch.equal(images[t], image) and {k: statuses[t][k] for k in lc.STATUS} == {k: status[k] for k in lc.STATUS}, t
        for k in ("theta_x", "theta_z"):
            assert statuses[t][k].dtype == np.float32 and np.array_equal(statuses[t][k].view(np.uint32), status[k].view(np.uint32)), (t, k)
        assert_member_equals((X, EI, EA, off), t, (x, ei, ea))
    five_union_steps(X, EI, EA, off, boundary, (501, 501), "points")
    with pytest.raises(ValueError, match="map 0 has more grains"):
        vz.samples_from_orientation_maps(dev[:, 0], dev[:, 1], G3, R3, tol, min_pixels=mp, grain_capacity=50, **kw)


def euler_maps(boundary):
    """Three EBSD maps of one shape: the recorded structure (periodic: frame 0 of the run; no-flux: the no-flux field), an
    orientation a grain, every map with its own draw of the 24 equivalents and signs per pixel -> (quats float64 [3, 4, ny, nx], tol)."""
    if boundary == "periodic":
        g = to.golden()
        field, grain_quats, tol = g["frame"] - 1, g["grain_quats"], to.GOLDEN_TOL
    else:
        field = np.load(os.path.join(GOLDEN, "grain_image_cfg1.npz"))["noflux__alpha_field"].astype(np.int32)
        grain_quats, tol = oc.random_quats(np.random.RandomState(7), 102), TOL      # (test_orient shows these more than 2 tol apart)
    maps = [oc.in_variants(grain_quats[:, field.reshape(-1)], np.random.RandomState(20 + t)).reshape(4, *field.shape) for t in range(3)]
    return np.stack(maps).astype(np.float64), tol


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
@torch.no_grad()
def test_samples_from_euler_maps(boundary, monkeypatch):
    quats, tol = cached(("euler maps", boundary), lambda: euler_maps(boundary))
    phi = [to_dev(a) for a in oc.bunge_from_quats(quats.transpose(1, 0, 2, 3))]                  # three [3, ny, nx] stacks
    kw = dict(span=6, patch_pixels=501 ** 2, grid="points", boundary=boundary)
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        counted = to.Counted(m)
        X, EI, EA, off, images, statuses = vz.samples_from_euler_maps(*phi, G3, R3, tol, **kw)
        assert counted.n == 3
    for t in range(3):
        x, ei, ea, image, status = vz.sample_from_euler_map(phi[0][t], phi[1][t], phi[2][t], G3[t], R3[t], tol, **kw)
        assert torch.equal(images[t], image) and {k: statuses[t][k] for k in lc.STATUS} == {k: status[k] for k in lc.STATUS}, t
        assert torch.equal(statuses[t]["mean_quats"].view(torch.int32), status["mean_quats"].view(torch.int32)), t
        for k in ("theta_x", "theta_z"):
            assert statuses[t][k].dtype == np.float32 and np.array_equal(statuses[t][k].view(np.uint32), status[k].view(np.uint32)), (t, k)
        assert_member_equals((X, EI, EA, off), t, (x, ei, ea))
    five_union_steps(X, EI, EA, off, boundary, (501, 501), "points")
    with pytest.raises(ValueError, match="map 0 has more grains"):
        vz.samples_from_euler_maps(*phi, G3, R3, tol, grain_capacity=50, **kw)
