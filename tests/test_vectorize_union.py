"""A stack of grain-ID images into one union rollout state (ggnn_image_junctions_traj / ggnn_junction_links_traj,
vectorize.graphs_from_images / samples_from_images / union_member) against the single-image calls and the restatement of
tests/vectorcheck_union.py.

The contract.  Every trajectory of the union, with its indices shifted back, equals the whole result of the single-image call
on its image BIT FOR BIT -- xy, triples, the three edge lists, the status, corner_grains and max_y --, the union equals the
restatement, and a union rollout started from samples_from_images leaves every trajectory torch.equal to its own rollout."""
import ctypes

import numpy as np
import pytest
import torch

import test_vectorize as tv
import test_vectorize_noflux as tn
import vectorcheck as vc
import vectorcheck_noflux as vn
import vectorcheck_union as vu
from helpers import product_models
from graingraphnn_amd import _lib
from graingraphnn_amd import vectorize as vz
from graingraphnn_amd.synthetic import EDGE_TYPES

DEV = "cuda"
GJ, JG, JJ = EDGE_TYPES
W = 7
BOUNDARIES = ("periodic", "noflux")

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def restated(key, images, n_grains, boundary, **kw):
    return cached(("union", key, boundary, tuple(sorted(kw.items()))), lambda: vu.vectorize(images, n_grains, boundary=boundary, **kw))


# ---- images ------------------------------------------------------------------------------------------------------------------

def seam_image(ny, nx):
    """Bricks, four rows of four; the junction under the first row's second brick has its boundary stepped, so that two
    windows a diagonal step apart carry its triple, and the image is rolled until they are (ny - 1, nx - 1) and (0, 0): the
    carriers of one junction wrap across both edges.  (32, 32) is test_vectorize's "seam"."""
    ry, cx = ny // 4, nx // 4
    even, odd = [0, cx, 2 * cx, 3 * cx], [cx // 2, cx // 2 + cx, cx // 2 + 2 * cx, cx // 2 + 3 * cx]
    plain, n = tv.bricks(ny, nx, [0, ry, 2 * ry, 3 * ry], [even, odd, even, odd])
    y, x = ry, cx // 2 + cx
    d = plain.copy()
    d[y, x + 1], d[y + 1, x] = plain[y - 1, x + 1], plain[y, x - 1]
    return np.roll(np.roll(d, -y, 0), -x, 1), n


def nine_bricks(ny, nx):
    return tv.bricks(ny, nx, [0, ny // 3, 2 * ny // 3], [[0, nx // 3, 2 * nx // 3], [5, 5 + nx // 3, 5 + 2 * nx // 3],
                                                          [8, 8 + nx // 3, 8 + 2 * nx // 3]])


def walls_with_a_grain(ny, nx):
    """walls_image with a grain two pixels wide at the top wall on the 2 | 3 boundary (the variant "two junctions close on a
    wall"): 8 grains, valid."""
    image, _ = tn.walls_image(ny, nx)
    image = image.copy()
    image[0:4, 11:13] = 8
    return image, 8


def two_bands(ny, nx):
    """Three grains over two: 6 grains with the boundary grain, 8 junctions, valid."""
    return tn.bands(ny, nx, [0, ny // 2, ny], [[10, 25], [18]])


def stack_of(boundary, ny, nx):
    """Three images that differ, with different grain counts.  Periodic: the walls image read as a torus (ids 2 .. 7), the
    seam image in the MIDDLE -- one of its junctions has its carriers at (ny - 1, nx - 1) and (0, 0), so a wrap that read
    the next or the previous image would change it --, nine bricks.  No-flux: the walls image, the one with a grain at the top
    wall, two bands."""
    if boundary == "periodic":
        made = [tn.walls_image(ny, nx), seam_image(ny, nx), nine_bricks(ny, nx)]
    else:
        made = [tn.walls_image(ny, nx), walls_with_a_grain(ny, nx), two_bands(ny, nx)]
    return [np.ascontiguousarray(m[0]) for m in made], [m[1] for m in made]


def one_grain(boundary, ny, nx):
    """An image that is one grain: id 1, or for no-flux id 2 inside the boundary grain."""
    return (np.ones((ny, nx), np.int32), 1) if boundary == "periodic" else (np.full((ny, nx), 2, np.int32), 2)


def fixture_stack(boundary):
    """Two different golden structures rasterised at 128 x 128."""
    if boundary == "periodic":
        return [tv.fixture_raster("graph_40", 128), tv.fixture_raster("generated_40_seed1", 128)], [118, 115]
    return [tn.fixture_raster("noflux_40_seed1", 128), tn.fixture_raster("noflux_80_seed3", 128)], [101, 400]


def rollout_stack(boundary):
    """Three valid 128 x 128 structures for a rollout: a golden raster, its transpose and its half turn (both keep the TL-BR
    diagonal of the rule, so a valid raster stays valid)."""
    image = tv.fixture_raster("graph_40", 128) if boundary == "periodic" else tn.fixture_raster("noflux_40_seed1", 128)
    n = 118 if boundary == "periodic" else 101
    return [np.ascontiguousarray(i) for i in (image, image.T, image[::-1, ::-1])], [n, n, n]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def hand_images():
    """Two 8 x 8 periodic images.  A: grain 1 around the blocks 2 (rows 2-4, columns 2-4) and 3 (rows 2-4, columns 5-6): the
    three meet above and below the 2 | 3 boundary, windows (1, 4) and (4, 4), three rows apart.  B: grain 1 around 2 (rows
    1-3, columns 1-3), 3 (rows 1-3, columns 4-6) and 4 (rows 4-6, columns 1-6) under both: windows (0, 3) = {1, 2, 3},
    (3, 0) = {1, 2, 4}, (3, 3) = {2, 3, 4}, (3, 6) = {1, 3, 4}: the four faces of a tetrahedron, every pair shared once."""
    a = np.ones((8, 8), np.int32)
    a[2:5, 2:5], a[2:5, 5:7] = 2, 3
    b = np.ones((8, 8), np.int32)
    b[1:4, 1:4], b[1:4, 4:7], b[4:7, 1:7] = 2, 3, 4
    return [a, b], [3, 4]


def test_restatement_of_a_union_worked_by_hand():
    images, n_grains = hand_images()
    v = vu.vectorize(images, n_grains)
    assert v["grain_off"] == [0, 3, 7] and v["joint_off"] == [0, 2, 6]
    assert v["triples"].tolist() == [[0, 1, 2], [0, 1, 2], [3, 4, 5], [3, 4, 6], [4, 5, 6], [3, 5, 6]]
    assert v["jj"][0].tolist() == [j for j in range(6) for _ in range(3)]
    assert v["jj"][1].tolist() == [1, 1, 1, 0, 0, 0, 3, 5, 4, 2, 5, 4, 2, 3, 5, 2, 3, 4]
    assert v["gj"][0].tolist() == v["triples"].reshape(-1).tolist() and np.array_equal(v["gj"][1], v["jj"][0])
    assert v["xy"].tolist() == [[5 / 8, 2 / 8], [5 / 8, 5 / 8], [4 / 8, 1 / 8], [1 / 8, 4 / 8], [4 / 8, 4 / 8], [7 / 8, 4 / 8]]
    zero = dict(n_quad_windows=0, n_merged_windows=0, n_invalid_pixels=0, n_open_pairs=0, overflow=0)
    assert v["status"] == [dict(zero, n_joint=2, n_present_grains=3), dict(zero, n_joint=4, n_present_grains=4)]
    assert v["counts"].tolist() == [49, 9, 6, 28, 9, 9, 18]
    # the capacity is the union's: it ends inside B, whose last pair of junctions is cut off with the links into it
    c = vu.vectorize(images, n_grains, joint_capacity=4)
    assert [s["overflow"] for s in c["status"]] == [0, 1] and c["joint_off"] == [0, 2, 6] and len(c["xy"]) == 4
    assert c["status"][0] == v["status"][0] and c["status"][1]["n_open_pairs"] == 4
    assert c["jj"][1].tolist() == [1, 1, 1, 0, 0, 0, 3, -1, -1, 2, -1, -1]
    assert np.array_equal(c["triples"], v["triples"][:4])
    # and an image that begins beyond it keeps nothing
    c = vu.vectorize(images[::-1], n_grains[::-1], joint_capacity=3)
    assert [s["overflow"] for s in c["status"]] == [1, 1] and c["status"][1]["n_open_pairs"] == 0 and c["jj"].shape == (2, 9)


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("ny,nx", [(32, 32), (24, 40)])
def test_the_stacks_show_what_they_were_made_for(boundary, ny, nx):
    images, n_grains = stack_of(boundary, ny, nx)
    assert len(set(n_grains)) == 3 and all(i.shape == (ny, nx) for i in images)
    assert not any(np.array_equal(a, b) for a, b in zip(images, images[1:] + images[:1]))
    v = restated((ny, nx), images, n_grains, boundary)
    if boundary == "periodic":   # the middle image's merged junction sits on both seams: representative (0, 0), carrier (-1, -1)
        s = v["status"][1]
        assert vc.is_valid(s) and s["n_merged_windows"] == 1 and s["n_joint"] == 32, s
        own = v["xy"][v["joint_off"][1]:v["joint_off"][2]]
        half = np.float32(0.5) * (np.float32(1) / np.float32(nx))
        assert np.all(own[0] == half) and (own <= 1.0).all()
    else:
        assert all(vn.is_valid(s) for s in v["status"]), v["status"]
        assert [s["n_joint"] for s in v["status"]] == [10, 12, 8]


def test_entry_points_validate_on_the_host():
    lib = _lib.load()
    assert lib.ggnn_version() == 26 == _lib.GGNN_ABI_VERSION
    assert {"ggnn_image_junctions_traj", "ggnn_junction_links_traj"} <= set(_lib.EXPORTED_SYMBOLS)
    assert lib.ggnn_image_junctions_traj(None, None) == -1 and lib.ggnn_junction_links_traj(None, None) == -1
    buf = (ctypes.c_int64 * 64)()                 # (host memory: refused before anything would be launched)
    p = ctypes.cast(buf, ctypes.c_void_p)
    seg = _lib.GGNN_JUNCTION_SEGMENT

    def call(**kw):
        A = _lib.JunctionTrajArgs(p, p, p, p, p, p, p, p, 4 * 3 * 32, 32, 32, 3, 16, 8, 1.0, 1.0 / 32, 2, 0)
        A.images = None                           # (so that a call that passes every other check still launches nothing)
        for k, v in kw.items():
            setattr(A, k, v)
        return lib.ggnn_image_junctions_traj(ctypes.byref(A), None)
    assert call() == -1
    for bad in (dict(grain_off=None), dict(pixel_counts=None), dict(xy=None), dict(triples=None), dict(edge_gj=None),
                dict(status=None), dict(workspace=None), dict(status=p.value + 4), dict(edge_gj=p.value + 4),
                dict(pixel_counts=p.value + 4), dict(grain_off=p.value + 4),
                dict(merge_radius=-1), dict(merge_radius=8), dict(nx=4), dict(ny=4), dict(nx=1 << 15), dict(ny=1 << 15),
                dict(n_grain=0), dict(n_grain=2 ** 31 - 2), dict(joint_capacity=0), dict(joint_capacity=2 ** 31 // 3 + 1),
                dict(offset=-0.5), dict(offset=2.0), dict(pitch=0.0), dict(pitch=float("nan")), dict(pitch=1.5),
                dict(boundary=2), dict(boundary=-1), dict(n_image=0), dict(n_image=-3),
                # one word a block: three images of 32 rows of one segment; of 33 rows for no-flux
                dict(workspace_bytes=4 * 96 - 1), dict(boundary=_lib.BC_NOFLUX, workspace_bytes=4 * 96),
                dict(boundary=_lib.BC_NOFLUX, workspace_bytes=4 * 99 - 1), dict(nx=257, workspace_bytes=4 * 192 - 1),
                dict(nx=256, boundary=_lib.BC_NOFLUX, workspace_bytes=4 * 3 * 33 * 2 - 1),
                # a grid beyond the launch limit, whatever the workspace
                dict(n_image=_lib.GGNN_JUNCTION_MAX_BLOCKS // 32 + 1, workspace_bytes=1 << 40),
                dict(n_image=_lib.GGNN_JUNCTION_MAX_BLOCKS + 1, workspace_bytes=1 << 40),
                dict(n_image=2 ** 62, workspace_bytes=1 << 40)):
        assert call(images=p, **bad) == -1, bad
    assert (256 + 1 + seg - 1) // seg == 2 and (257 + seg - 1) // seg == 2

    def links(**kw):
        A = _lib.LinkTrajArgs(p, p, p, p, p, 16, 8, 24, 3)
        A.triples = None
        for k, v in kw.items():
            setattr(A, k, v)
        return lib.ggnn_junction_links_traj(ctypes.byref(A), None)
    assert links() == -1
    for bad in (dict(rowptr=None), dict(col=None), dict(edge_jj=None), dict(status=None), dict(status=p.value + 4),
                dict(edge_jj=p.value + 4), dict(n_grain=0), dict(joint_capacity=0), dict(E_cap=-1), dict(E_cap=2 ** 31 - 1),
                dict(n_image=0), dict(n_image=_lib.GGNN_JUNCTION_MAX_BLOCKS + 1)):
        assert links(triples=p, **bad) == -1, bad


def test_header_binding_and_struct_sizes_agree():
    import re
    from helpers import ROOT
    import os
    src = open(os.path.join(ROOT, "include", "ggnn.h")).read()
    assert re.search(r"#define GGNN_ABI_VERSION 26\b", src) and _lib.GGNN_ABI_VERSION == 26
    assert f"#define GGNN_JUNCTION_MAX_BLOCKS (1 << {_lib.GGNN_JUNCTION_MAX_BLOCKS.bit_length() - 1})" in src
    for struct, mirror in (("ggnn_junction_traj_args", _lib.JunctionTrajArgs), ("ggnn_link_traj_args", _lib.LinkTrajArgs)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+)\s*[,;]", body)
        assert names == [f[0] for f in mirror._fields_], (struct, names)
    assert ctypes.sizeof(_lib.JunctionTrajArgs) == 9 * 8 + 5 * 8 + 4 * 4 and ctypes.sizeof(_lib.LinkTrajArgs) == 5 * 8 + 4 * 8
    # the single-image structs are as they were
    assert ctypes.sizeof(_lib.JunctionArgs) == 8 * 8 + 4 * 8 + 4 * 4 and ctypes.sizeof(_lib.LinkArgs) == 5 * 8 + 3 * 8
    assert _lib.JunctionTrajArgs.boundary.offset == _lib.JunctionTrajArgs.merge_radius.offset + 4


def test_python_entry_points_refuse_what_they_cannot_take():
    host = torch.ones(2, 8, 8, dtype=torch.int32)
    with pytest.raises(_lib.GGNNError, match="device tensor"):
        vz.graphs_from_images(host, [1, 1])
    with pytest.raises(_lib.GGNNError, match="one shape a stack"):
        vz.graphs_from_images([host[0], torch.ones(8, 9, dtype=torch.int32)], [1, 1])
    with pytest.raises(_lib.GGNNError, match="boundary must be"):
        vz.graphs_from_images(host, [1, 1], boundary="walls")
    with pytest.raises(_lib.GGNNError, match="one angle per grain"):
        vz.samples_from_images(host, [np.zeros(2), np.zeros(2)], [np.zeros(2), np.zeros(3)], 2.0, 0.4, span=6)
    with pytest.raises(_lib.GGNNError, match="one value per image"):
        vz.samples_from_images(host, [np.zeros(2), np.zeros(2)], [np.zeros(2), np.zeros(2)], [2.0, 3.0, 4.0], 0.4, span=6)
    from graingraphnn_amd.synthetic import span_for
    pairs = [(2.0, 0.4), (9.0, 1.9), (0.6, 0.3), (5.0, 1.0)]
    spans = [span_for(g, r) for g, r in pairs]
    other = next(i for i, s in enumerate(spans) if s != spans[0])   # (the grid's spans differ across it)
    with pytest.raises(_lib.GGNNError, match="pass span="):
        vz.samples_from_images(host, [np.zeros(2), np.zeros(2)], [np.zeros(2), np.zeros(2)], [pairs[0][0], pairs[other][0]],
                               [pairs[0][1], pairs[other][1]])
    # union_member on a result made by hand: indices come back local, -1 stays -1
    res = {"xy": torch.arange(12.0).view(6, 2), "triples": torch.tensor([[0, 1, 2]] * 2 + [[3, 4, 5]] * 4, dtype=torch.int32),
           "edge_index_dict": {GJ: torch.stack([torch.tensor([0, 1, 2] * 2 + [3, 4, 5] * 4), torch.arange(6).repeat_interleave(3)]),
                               JJ: torch.stack([torch.arange(6).repeat_interleave(3), torch.tensor([1, 1, 1, 0, 0, 0] + [3, -1, 5] * 4)])},
           "status": ["a", "b"], "traj_offsets": {"grain": [0, 3, 6], "joint": [0, 2, 6]}}
    xy, triples, ei, status = vz.union_member(res, 1)
    assert status == "b" and xy.tolist() == res["xy"][2:].tolist() and triples.tolist() == [[0, 1, 2]] * 4 and triples.dtype == torch.int32
    assert ei[GJ].tolist() == [[0, 1, 2] * 4, [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]] and torch.equal(ei[JG], ei[GJ].flip(0))
    assert ei[JJ].tolist() == [[0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3], [1, -1, 3] * 4]
    with pytest.raises(_lib.GGNNError, match="trajectories"):
        vz.union_member(res, 2)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

def to_dev(images):
    return torch.from_numpy(np.stack(images).astype(np.int32)).to(DEV)


def assert_same_graph(got, want, what):
    """Two results in graph_from_image's shape, bit for bit."""
    assert len(got) == len(want) == (6 if len(want) > 4 else 4), what
    (xy, triples, ei, status), (xy1, triples1, ei1, status1) = got[:4], want[:4]
    assert status == status1, (what, status, status1)
    assert xy.dtype == xy1.dtype == torch.float32 and xy.shape == xy1.shape and torch.equal(xy.view(torch.int32), xy1.view(torch.int32)), what
    assert triples.dtype == triples1.dtype == torch.int32 and torch.equal(triples, triples1), what
    for et in EDGE_TYPES:
        assert ei[et].dtype == torch.int64 and ei[et].is_contiguous() and torch.equal(ei[et], ei1[et]), (what, et)
    assert tuple(got[4:]) == tuple(want[4:]), (what, got[4:], want[4:])          # corner_grains and max_y


def assert_equals_restatement(res, v, what):
    n = len(v["xy"])
    assert res["status"] == v["status"], (what, res["status"], v["status"])
    assert res["traj_offsets"]["grain"] == v["grain_off"] and res["traj_offsets"]["joint"] == [min(o, n) for o in v["joint_off"]]
    assert np.array_equal(res["xy"].cpu().numpy().view(np.uint32), v["xy"].view(np.uint32)), what
    assert np.array_equal(res["triples"].cpu().numpy(), v["triples"]), what
    ei = res["edge_index_dict"]
    assert np.array_equal(ei[GJ].cpu().numpy(), v["gj"]) and np.array_equal(ei[JG].cpu().numpy(), v["gj"][::-1]), what
    assert np.array_equal(ei[JJ].cpu().numpy(), v["jj"]), what
    if "corner_grains" in v:
        assert res["corner_grains"] == v["corner_grains"] and res["max_y"] == float(v["max_y"]), what


def check_members(images, n_grains, boundary, members=None, **kw):
    """graphs_from_images(strict=False) of the stack; the listed members (all) equal their own single-image calls."""
    dev = to_dev(images)
    res = vz.graphs_from_images(dev, n_grains, strict=False, boundary=boundary, **kw)
    for t in (range(len(images)) if members is None else members):
        own = vz.graph_from_image(dev[t], n_grains[t], strict=False, boundary=boundary, **kw)
        assert_same_graph(vz.union_member(res, t), own, (boundary, t))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("ny,nx", [(32, 32), (24, 40)])
def test_every_trajectory_equals_the_single_image_call(boundary, ny, nx):
    images, n_grains = stack_of(boundary, ny, nx)
    for grid in ("cells", "points"):
        res = check_members(images, n_grains, boundary, grid=grid)
        if grid == "cells":
            assert_equals_restatement(res, restated((ny, nx), images, n_grains, boundary), (boundary, ny, nx))
    # a list of images and n_grains=None (the largest id of every image) give the same; so does every order of the stack
    dev = to_dev(images)
    again = vz.graphs_from_images(list(dev), boundary=boundary, strict=False)
    assert again["traj_offsets"] == res["traj_offsets"] and torch.equal(again["triples"], res["triples"])
    check_members(images[::-1], n_grains[::-1], boundary)
    # B = 1
    for t in range(3):
        check_members(images[t:t + 1], n_grains[t:t + 1], boundary)
        # ... and at the entry points: the one-image union's words and counts are the single call's
        one = vz._vectorize_union(dev[t:t + 1], n_grains[t:t + 1], "cells", 2, None, boundary)
        own = vz._vectorize(dev[t], n_grains[t], "cells", 2, None, boundary)
        words, seven = one["status"].tolist(), own["status"][:7].tolist()
        assert words[:7] == seven and words[7:9] == [0, seven[0]], (boundary, t, words, seven)     # the row, then joint_off
        assert own["counts"].numel() == n_grains[t] + 1 and torch.equal(one["counts"], own["counts"][1:]), (boundary, t)
    if boundary == "noflux":   # all three are valid: strict passes
        assert vz.graphs_from_images(dev, n_grains, boundary=boundary)["status"] == res["status"]


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("nx", [255, 256, 257])
def test_strips_across_the_segment_edge(boundary, nx):
    """The block -> (image, row, segment) mapping where a row is one segment, exactly one, and two."""
    image, n_grain = tn.strip(nx)
    images, n_grains = [image, np.ascontiguousarray(image[::-1])], [n_grain, n_grain]
    res = check_members(images, n_grains, boundary)
    assert_equals_restatement(res, restated(("strip", nx), images, n_grains, boundary), (boundary, nx))


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_an_id_is_judged_by_its_own_image(boundary):
    """Id 8 is a grain of image 0 and one above image 1's count: image 1's n_invalid_pixels alone shows it."""
    if boundary == "noflux":
        a, b = walls_with_a_grain(32, 32), tn.walls_image(32, 32)
    else:
        a, b = nine_bricks(32, 32), tn.walls_image(32, 32)           # (9 grains; ids 2 .. 7 of 7 on the torus)
    b = (b[0].copy(), b[1])
    b[0][15, 3] = 8
    assert (a[0] == 8).any() and a[1] >= 8 and b[1] == 7
    images, n_grains = [a[0], b[0]], [a[1], b[1]]
    res = check_members(images, n_grains, boundary)
    assert res["status"][0]["n_invalid_pixels"] == 0 and res["status"][1]["n_invalid_pixels"] == 1
    assert vz.status_is_valid(res["status"][0], boundary)       # (nine bricks are a valid torus, the walls with a grain a valid box)
    with pytest.raises(ValueError, match=rf"1 of 2 images are not valid {boundary}.*image 1: \{{.*'n_invalid_pixels': 1") as err:
        vz.graphs_from_images(to_dev(images), n_grains, boundary=boundary)
    assert "image 0" not in str(err.value)


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_a_one_grain_image_between_two_real_ones(boundary):
    images, n_grains = stack_of(boundary, 24, 40)
    images[1], n_grains[1] = one_grain(boundary, 24, 40)
    res = check_members(images, n_grains, boundary)
    oj = res["traj_offsets"]["joint"]
    assert oj[1] == oj[2] and 0 < oj[1] < oj[3]
    assert res["status"][1] == dict(zip(vz.STATUS_WORDS, (0, 0, 0, 0, 0, 1, 0)))
    assert_equals_restatement(res, restated("one grain", images, n_grains, boundary), boundary)


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("at", [0, 2])
def test_a_one_grain_image_first_or_last(boundary, at):
    """The image without junctions at either end of the stack: joint_off begins, or ends, with two equal offsets."""
    images, n_grains = stack_of(boundary, 24, 40)
    images[at], n_grains[at] = one_grain(boundary, 24, 40)
    res = check_members(images, n_grains, boundary)
    oj = res["traj_offsets"]["joint"]
    assert oj[at] == oj[at + 1] and oj[3] > 0
    assert_equals_restatement(res, restated(("one grain", at), images, n_grains, boundary), (boundary, at))


def guarded_call(images, n_grains, boundary, cap):
    """The entry points themselves on guarded arrays -> (xy, triples, gj, jj, status, counts, ws) with 16 guard words of -7
    behind each, n_blocks."""
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
    gj = torch.full((6 * cap + 16,), -7, dtype=torch.int64, device=DEV)
    jj = torch.full((6 * cap + 16,), -7, dtype=torch.int64, device=DEV)
    status = torch.full((B * W + B + 1 + 16,), -7, dtype=torch.int64, device=DEV)
    counts = torch.full((n_total + 16,), -7, dtype=torch.int64, device=DEV)
    ws = torch.full((n_blocks + 16,), -7, dtype=torch.int32, device=DEV)
    A = _lib.JunctionTrajArgs(dev.data_ptr(), off.data_ptr(), counts.data_ptr(), xy.data_ptr(), triples.data_ptr(), gj.data_ptr(),
                              status.data_ptr(), ws.data_ptr(), 4 * n_blocks, nx, ny, B, n_total, cap, 1.0,
                              float(np.float32(1) / np.float32(nx)), 2, vz.BOUNDARIES[boundary])
    _lib.check(lib.ggnn_image_junctions_traj(ctypes.byref(A), _lib.current_stream()), "ggnn_image_junctions_traj")
    rows = gj[:6 * cap].view(2, 3 * cap)
    n = min(int(status[B * W + B]), cap)
    table = torch.stack([rows[1, :3 * n], rows[0, :3 * n]]).contiguous()          # joint -> grain, the junctions written
    csr = be.build_csr_batch([(table, cap, n_total)])[0]
    L = _lib.LinkTrajArgs(triples.data_ptr(), csr.rowptr.data_ptr(), csr.col.data_ptr(), jj.data_ptr(), status.data_ptr(),
                          n_total, cap, csr.col.numel(), B)
    _lib.check(lib.ggnn_junction_links_traj(ctypes.byref(L), _lib.current_stream()), "ggnn_junction_links_traj")
    A.workspace_bytes = 4 * n_blocks - 1                                           # (the exact size was accepted above)
    assert lib.ggnn_image_junctions_traj(ctypes.byref(A), _lib.current_stream()) == -1
    return (xy, triples, gj, jj, status, counts, ws), n_blocks


@pytest.mark.gpu
@pytest.mark.parametrize("boundary,ny,nx", [("periodic", 32, 32), ("noflux", 24, 40)])
def test_the_capacity_ends_inside_the_second_image(boundary, ny, nx):
    images, n_grains = stack_of(boundary, ny, nx)
    full = restated((ny, nx), images, n_grains, boundary)
    B, n_total = 3, sum(n_grains)
    for cap in (full["joint_off"][1] + 3, full["joint_off"][3] + 4):
        v = restated((ny, nx), images, n_grains, boundary, joint_capacity=cap)
        inside = cap < full["joint_off"][3]
        assert [s["overflow"] for s in v["status"]] == ([0, 1, 1] if inside else [0, 0, 0])
        (xy, triples, gj, jj, status, counts, ws), n_blocks = guarded_call(images, n_grains, boundary, cap)
        n = min(cap, full["joint_off"][3])
        words = status.tolist()
        assert [dict(zip(vz.STATUS_WORDS, words[b * W:(b + 1) * W])) for b in range(B)] == v["status"]
        assert words[B * W:B * W + B + 1] == full["joint_off"] and words[B * W + B + 1:] == [-7] * 16
        assert np.array_equal(xy[:2 * n].cpu().numpy().view(np.uint32), v["xy"].reshape(-1).view(np.uint32))
        assert np.array_equal(triples[:3 * n].cpu().numpy(), v["triples"].reshape(-1))
        assert bool((xy[2 * n:] == -7).all()) and bool((triples[3 * n:] == -7).all())          # between n_joint and the capacity too
        for lists, want in ((gj, v["gj"]), (jj, v["jj"])):
            rows = lists[:6 * cap].view(2, 3 * cap)
            assert np.array_equal(rows[:, :3 * n].cpu().numpy(), want)
            assert bool((rows[:, 3 * n:] == -7).all()) and bool((lists[6 * cap:] == -7).all())
        assert np.array_equal(counts[:n_total].cpu().numpy(), v["counts"]) and bool((counts[n_total:] == -7).all())
        assert bool((ws[n_blocks:] == -7).all())
    # through the Python call: image 0's slice is intact, the images from 1 on report the overflow
    cap = full["joint_off"][1] + 3
    res = check_members(images, n_grains, boundary, members=[0], joint_capacity=cap)
    assert [s["overflow"] for s in res["status"]] == [0, 1, 1]
    assert_equals_restatement(res, restated((ny, nx), images, n_grains, boundary, joint_capacity=cap), boundary)
    bad = [b for b, s in enumerate(res["status"]) if not vz.status_is_valid(s, boundary)]
    assert bad[-2:] == [1, 2]                                   # (the walls image read as a torus is no valid structure either)
    with pytest.raises(ValueError, match=f"{len(bad)} of 3 images") as err:
        vz.graphs_from_images(to_dev(images), n_grains, boundary=boundary, joint_capacity=cap)
    assert all(f"image {b}: " in str(err.value) for b in bad) and f"joint_capacity {cap}" in str(err.value)


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_captured_graph_gives_the_same_bits(boundary):
    images, n_grains = stack_of(boundary, 24, 40)
    v = restated((24, 40), images, n_grains, boundary)
    dev = vz._stack(to_dev(images))
    off = vz.grain_offsets(n_grains, DEV)
    eager = vz._vectorize_union(dev, n_grains, "cells", 2, None, boundary, grain_off=off)   # (also the warm-up of the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = vz._vectorize_union(dev, n_grains, "cells", 2, None, boundary, grain_off=off)
    for _ in range(2):                                                           # (a replay starts from its own zeroed status)
        graph.replay()
    torch.cuda.synchronize()
    for k in ("xy", "triples", "gj", "jj", "status", "counts"):
        assert torch.equal(held[k], eager[k]), k
    words = held["status"].tolist()
    assert [dict(zip(vz.STATUS_WORDS, words[b * W:(b + 1) * W])) for b in range(3)] == v["status"]
    assert words[3 * W:3 * W + 4] == v["joint_off"]
    n = v["joint_off"][-1]
    assert np.array_equal(held["xy"][:n].cpu().numpy().view(np.uint32), v["xy"].view(np.uint32))
    assert np.array_equal(held["counts"].cpu().numpy(), v["counts"])


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_rasters_of_two_golden_structures(boundary):
    images, n_grains = fixture_stack(boundary)
    res = check_members(images, n_grains, boundary)
    assert_equals_restatement(res, restated("fixtures", images, n_grains, boundary), boundary)
    assert res["status"][0]["n_joint"] == (236 if boundary == "periodic" else 198)


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
@torch.no_grad()
def test_samples_into_a_union_rollout(boundary):
    """samples_from_images on three structures with their own G and R: every trajectory's slice is sample_from_image's of its
    image; three static steps of the union rollout leave every trajectory as its own rollout does; an eventful step runs."""
    from graingraphnn_amd import GrainRollout
    images, n_grains = rollout_stack(boundary)
    dev = to_dev(images)
    rs = np.random.RandomState(11)
    theta_x = [rs.uniform(0, np.pi / 2, n) for n in n_grains]
    theta_z = [rs.uniform(0, np.pi / 2, n) for n in n_grains]
    G, R = [2.0, 3.5, 1.2], [0.4, 0.9, 0.25]
    X, EI, EA, off = vz.samples_from_images(dev, theta_x, theta_z, G, R, span=6, boundary=boundary)
    og, oj = off["grain"], off["joint"]
    assert og == [0] + list(np.cumsum(n_grains)) and X["grain"].shape == (og[-1], 11) and X["joint"].shape == (oj[-1], 8)
    kw = dict(boundary="noflux", max_y=vz.image_max_y(128, 128, "cells")) if boundary == "noflux" else {}
    Rm, Cm = product_models(10020, 1.0, DEV)
    own_after = []
    for t in range(3):
        x, ei, ea = vz.sample_from_image(dev[t], theta_x[t], theta_z[t], G[t], R[t], span=6, boundary=boundary)
        assert torch.equal(X["grain"][og[t]:og[t + 1]], x["grain"]) and torch.equal(X["joint"][oj[t]:oj[t + 1]], x["joint"]), t
        for et in EDGE_TYPES:
            shift = torch.tensor([[off[et[0]][t]], [off[et[2]][t]]], device=DEV)
            assert torch.equal(EI[et][:, 3 * oj[t]:3 * oj[t + 1]] - shift, ei[et]), (t, et)
            assert torch.equal(EA[et][3 * oj[t]:3 * oj[t + 1]], ea[et]), (t, et)
        ro = GrainRollout(Rm, Cm, x, ei, ea, 6, refresh_centres=True, **kw)
        for _ in range(3):
            ro.step()
        assert not ro.range_exceeded()
        own_after.append({k: v.clone() for k, v in ro.x.items()})
    first = {k: v.clone() for k, v in X.items()}
    union_kw = dict(kw, traj_offsets=off) if boundary == "noflux" else kw
    ro = GrainRollout(Rm, Cm, X, EI, EA, 6, refresh_centres=True, **union_kw)
    for _ in range(3):
        ro.step()
    assert not ro.range_exceeded() and not torch.equal(ro.x["joint"], first["joint"])
    for t in range(3):
        assert torch.equal(ro.x["grain"][og[t]:og[t + 1]], own_after[t]["grain"]), t
        assert torch.equal(ro.x["joint"][oj[t]:oj[t + 1]], own_after[t]["joint"]), t
    # one eventful step on the union, from the same first state
    X2 = {k: v.clone() for k, v in first.items()}
    ro = GrainRollout(Rm, Cm, X2, {et: v.clone() for et, v in EI.items()}, {et: v.clone() for et, v in EA.items()}, 6,
                      refresh_centres=True, **union_kw)
    ro.enable_events({"grain": np.ones((og[-1], 1)), "joint": np.ones((oj[-1], 1))}, 1e-4, 0.6, traj_offsets=off)
    pred = ro.step_events()[0]
    assert all(bool(torch.isfinite(t).all()) for t in pred.values())
