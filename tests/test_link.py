"""Grain ids that persist across a sequence of labelled maps (ggnn_link_labels, vectorize.link_labels / label_sequence /
samples_from_orientation_sequence) against the numpy restatement of tests/linkcheck.py, and the restatement against hand-drawn
stacks and the recorded phase-field sequence.

The contract.  KERNELS against RESTATEMENT: the relabelled frames, gid, pred, first_frame, last_frame, theta and every status
word equal, bit for bit, with canary words round every output and the workspace untouched.  RESTATEMENT against the RULE: one
hand-drawn stack per clause of include/ggnn.h's rule; on the seven frames of pf_frames_cfg1.npz, each labelled on its own by
tests/labelcheck.py, it gives the recorded frames renumbered in frame 0's raster order in every pixel, clean, and the recorded
table of differing pixels under the two noise settings."""
import ctypes
import os

import numpy as np
import pytest
import torch

import labelcheck as lc
import linkcheck as lk
import trackcheck as tc
import vectorcheck_union as vu
from helpers import GOLDEN, ROOT
from graingraphnn_amd import _lib
from graingraphnn_amd import vectorize as vz

DEV = "cuda"
BOUNDARIES = ("periodic", "noflux")
FW, GW = _lib.GGNN_LINK_FRAME_WORDS, _lib.GGNN_LINK_GLOBAL_WORDS
GONE = [0, 0, 0, 1, 6, 11]                       # grains gone per pair of recorded frames
CANDIDATES = [8, 8, 8, 9, 9, 11]                 # the most grains of frame t - 1 that one grain of frame t overlaps
NOISE = {0.04: (1, [131, 126, 153, 151, 125, 127, 131]), 0.10: (2, [423, 442, 440, 422, 425, 448, 394])}   # d: seed0, differing
# DESIGN 8m's table of the recorded sequence: matched, junctions, labels 0 / 1 / unlabelled, grains eliminated
TABLE = [(234, 236, 698, 2, 8, 0), (234, 236, 698, 2, 8, 0), (226, 236, 658, 10, 40, 0), (206, 236, 568, 26, 114, 1),
         (188, 234, 506, 22, 174, 6)]

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def f32(a):
    return np.asarray(a, np.float32)


def restated(key, **kw):
    """The restatement of a named input, computed once and left unchanged."""
    return cached(("link", key), lambda: lk.link(**kw))


# ---- hand-drawn stacks: one per clause of the rule -> (keywords of link, check(result)) --------------------------------------

TOL = np.float32(0.25)


def stack(*rows, height=3):
    """One frame per row of ids, every row repeated `height` times."""
    return np.stack([np.tile(np.array(r, np.int32), (height, 1)) for r in rows])


def flat(r, t):
    return r["frames"][t][0].tolist()


def words(r, t):
    return tuple(r["status"][t][k] for k in lk.FRAME_WORDS)


def hand_cases():
    c = {}

    def identity(r):
        assert flat(r, 1) == [1, 1, 1, 2, 2, 2] and r["pred"][1].tolist() == [1, 2] and r["gid"][1].tolist() == [1, 2]
        assert words(r, 1) == (2, 2, 0, 0, 0, 0) and words(r, 0) == (2, 0, 0, 0, 0, 0) and r["n_global"] == 2 == r["n_grain"]
        assert r["first_frame"].tolist()[:2] == [0, 0] and r["last_frame"].tolist()[:2] == [1, 1]
    c["identity"] = (dict(labels=stack([1, 1, 1, 2, 2, 2], [1, 1, 1, 2, 2, 2]), n_local=[2, 2]), identity)

    def permuted(r):
        assert flat(r, 1) == [1, 1, 1, 2, 2, 2] and r["pred"][1].tolist() == [2, 1] and r["gid"][1].tolist() == [2, 1]
    c["a permuted numbering of frame 1"] = (dict(labels=stack([1, 1, 1, 2, 2, 2], [2, 2, 2, 1, 1, 1]), n_local=[2, 2]), permuted)

    def vanishing(r):
        assert flat(r, 1) == [1, 1, 1, 3, 3, 3] and words(r, 1) == (2, 2, 0, 0, 1, 0) and r["n_global"] == 3
        assert r["last_frame"].tolist()[:3] == [1, 0, 1]
    c["a vanishing grain"] = (dict(labels=stack([1, 1, 2, 2, 3, 3], [1, 1, 1, 2, 2, 2]), n_local=[3, 2]), vanishing)

    def pinched(r):
        assert flat(r, 1) == [1, 1, 1, 1, 3, 3, 2, 2] and words(r, 1) == (3, 2, 1, 1, 0, 0) and r["n_global"] == 3
        assert r["pred"][1].tolist() == [1, -1, 2] and r["first_frame"].tolist()[:3] == [0, 0, 1]
    c["pinched in two: the larger part keeps the id"] = (dict(labels=stack([1, 1, 1, 1, 1, 1, 2, 2], [1, 1, 1, 1, 2, 2, 3, 3]), n_local=[2, 3]),
                                                        pinched)

    def pinched_larger_second(r):
        assert flat(r, 1) == [3, 3, 1, 1, 1, 1, 2, 2] and r["pred"][1].tolist() == [-1, 1, 2] and words(r, 1) == (3, 2, 1, 1, 0, 0)
    c["pinched in two: the larger part has the larger id"] = (dict(labels=stack([1, 1, 1, 1, 1, 1, 2, 2], [1, 1, 2, 2, 2, 2, 3, 3]),
                                                                   n_local=[2, 3]), pinched_larger_second)

    def pinched_equal(r):
        assert flat(r, 1) == [1, 1, 1, 3, 3, 3, 2, 2] and r["pred"][1].tolist() == [1, -1, 2] and words(r, 1) == (3, 2, 1, 1, 0, 0)
    c["pinched in equal parts: the smaller b"] = (dict(labels=stack([1, 1, 1, 1, 1, 1, 2, 2], [1, 1, 1, 2, 2, 2, 3, 3]), n_local=[2, 3]),
                                                 pinched_equal)

    def tie(r):
        assert flat(r, 1) == [1, 1, 2, 2, 2, 2] and r["pred"][1].tolist() == [1, 2, -1] and words(r, 1) == (2, 2, 0, 0, 1, 0)
        assert r["last_frame"].tolist()[:3] == [1, 1, 0]
    c["an argmax tie: the smaller a"] = (dict(labels=stack([1, 1, 3, 3, 2, 2], [1, 1, 2, 2, 2, 2]), n_local=[3, 2]), tie)

    def fresh(r):
        assert flat(r, 1) == [1, 1, 3, 3, 4, 4, 2, 0] and flat(r, 2) == [1, 1, 3, 3, 4, 4, 2, 5]
        assert words(r, 1) == (4, 2, 2, 0, 0, 0) and words(r, 2) == (5, 4, 1, 0, 0, 0) and r["n_global"] == 5
        assert r["first_frame"].tolist()[:5] == [0, 0, 1, 1, 2] and r["last_frame"].tolist()[:5] == [2] * 5
        assert r["gid"][2].tolist() == [1, 3, 4, 2, 5] and r["pred"][2].tolist() == [1, 2, 3, 4, -1]
    c["fresh grains in frames 1 and 2, numbered by frame and then id"] = (
        dict(labels=stack([1, 1, 0, 0, 0, 0, 2, 2], [1, 1, 2, 2, 3, 3, 4, 0], [1, 1, 2, 2, 3, 3, 4, 5]), n_local=[2, 4, 5]), fresh)

    def back(r):      # grain 2 is gone in frame 1; what stands in its place in frame 2 is a new grain
        assert flat(r, 1) == [1, 1, 1, 0, 0, 0] and flat(r, 2) == [1, 1, 1, 3, 3, 3] and r["n_global"] == 3
        assert words(r, 1) == (1, 1, 0, 0, 1, 0) and words(r, 2) == (2, 1, 1, 0, 0, 0)
        assert r["first_frame"].tolist()[:3] == [0, 0, 2] and r["last_frame"].tolist()[:3] == [2, 0, 2]
    c["absent in one frame: back as a fresh grain"] = (dict(labels=stack([1, 1, 1, 2, 2, 2], [1, 1, 1, 0, 0, 0], [1, 1, 1, 2, 2, 2]),
                                                            n_local=[2, 1, 2]), back)

    overlap3 = stack([0, 0, 0, 1, 0, 0], [0, 0, 0, 1, 1, 1])

    def at_overlap(r):
        assert flat(r, 1) == [0, 0, 0, 1, 1, 1] and words(r, 1) == (1, 1, 0, 0, 0, 0) and r["n_global"] == 1
    c["min_overlap at the overlap"] = (dict(labels=overlap3, n_local=[1, 1], min_overlap=3), at_overlap)

    def above_overlap(r):
        assert flat(r, 1) == [0, 0, 0, 2, 2, 2] and words(r, 1) == (1, 0, 1, 0, 1, 0) and r["n_global"] == 2
    c["min_overlap one above the overlap"] = (dict(labels=overlap3, n_local=[1, 1], min_overlap=4), above_overlap)

    def means_of(*frames):      # [T, 1, 2]
        return f32(frames)[:, None, :]

    def second_choice(r):
        assert flat(r, 1) == [2] * 6 and r["pred"][1].tolist() == [2, -1] and words(r, 1) == (1, 1, 0, 0, 1, 0)
        assert r["theta"][:, :2].tolist() == [[0.5, 1.0]]
    c["match_tol excludes the majority candidate"] = (dict(labels=stack([1, 1, 1, 1, 2, 2], [1, 1, 1, 1, 1, 1]), n_local=[2, 1],
                                                           means=means_of([0.5, 1.0], [1.0, 0.0]), match_tol=0.1), second_choice)

    def without_gate(r):
        assert flat(r, 1) == [1] * 6 and r["pred"][1].tolist() == [1, -1]
    c["the same without match_tol"] = (dict(labels=stack([1, 1, 1, 1, 2, 2], [1, 1, 1, 1, 1, 1]), n_local=[2, 1],
                                            means=means_of([0.5, 1.0], [1.0, 0.0])), without_gate)

    two = stack([1, 1, 1, 2, 2, 2], [1, 1, 1, 2, 2, 2])

    def exactly_tol(r):
        assert flat(r, 1) == [1, 1, 1, 2, 2, 2] and words(r, 1) == (2, 2, 0, 0, 0, 0)
    c["a difference of exactly match_tol matches"] = (dict(labels=two, n_local=[2, 2], means=means_of([0.0, 1.0], [TOL, 1.0]), match_tol=TOL),
                                                      exactly_tol)

    def beyond_tol(r):
        assert flat(r, 1) == [3, 3, 3, 2, 2, 2] and words(r, 1) == (2, 1, 1, 0, 1, 0)
        assert r["theta"][0, :3].tolist() == [0.0, 1.0, float(np.nextafter(TOL, np.float32(1)))]
    c["nextafter(match_tol) does not match"] = (dict(labels=two, n_local=[2, 2], means=means_of([0.0, 1.0], [np.nextafter(TOL, np.float32(1)), 1.0]),
                                                     match_tol=TOL), beyond_tol)

    def zeros(r):     # the unfilled pixels of frame 1 lie on grain 1 of frame 0, those of frame 0 under grain 2 of frame 1
        assert flat(r, 0) == [1, 1, 0, 0, 2, 2] and flat(r, 1) == [0, 1, 1, 1, 1, 2] and words(r, 1) == (2, 2, 0, 0, 0, 0)
        assert r["pred"][1].tolist() == [2, 1]        # (were 0 a grain, it would hold the most pixels of frame 1's grain 2)
    c["pixel 0 neither votes nor changes"] = (dict(labels=stack([1, 1, 0, 0, 2, 2], [0, 2, 2, 2, 2, 1]), n_local=[2, 2], min_overlap=3), zeros)

    def walls(r):
        assert flat(r, 0) == [1, 2, 2, 3, 3, 3] and flat(r, 1) == [1, 1, 2, 2, 3, 3] and r["n_global"] == 2 and r["n_grain"] == 3
        assert r["gid"][1].tolist() == [3, 2] and r["pred"][1].tolist() == [3, 2] and r["overflow"] == 0
    c["no-flux: id 1 stays 1 and the grains start at 2"] = (dict(labels=stack([1, 2, 2, 3, 3, 3], [1, 1, 3, 3, 2, 2]), n_local=[2, 2],
                                                                 boundary="noflux"), walls)

    def one_frame(r):
        assert flat(r, 0) == [2, 2, 1, 1, 0, 3] and r["n_global"] == 3 and words(r, 0) == (3, 0, 0, 0, 0, 0) and r["candidates"] == []
        assert r["first_frame"].tolist() == [0, 0, 0] and r["gid"].tolist() == [[1, 2, 3]]
    c["T = 1"] = (dict(labels=stack([2, 2, 1, 1, 0, 3]), n_local=[3]), one_frame)
    return c


HAND = hand_cases()


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_drawn_clauses_of_the_rule(name):
    kw, check = HAND[name]
    r = restated(("hand", name), **kw)
    check(r)
    assert r["overflow"] == 0 and r["frames"].dtype == np.int32 and all(s["n_vote_overflow"] == 0 for s in r["status"])
    for t in range(len(r["frames"])):          # an unfilled pixel stays 0 and nothing else becomes 0
        assert np.array_equal(r["frames"][t] == 0, kw["labels"][t] == 0), t


def test_the_restatement_counts_what_it_cannot_place():
    labels = stack([1, 1, 2, 2, 3, 3], [1, 1, 2, 2, 3, -4])
    r = lk.link(labels, [3, 3], local_capacity=2, global_capacity=2)          # id 3 lies beyond the rows, and so does n_local
    assert r["frames"][0][0].tolist() == [1, 1, 2, 2, 0, 0] and r["frames"][1][0].tolist() == [1, 1, 2, 2, 0, 0]
    assert r["overflow"] == 2 + 3 * 4 and r["n_global"] == 2
    r = lk.link(stack([1, 1, 0, 0, 0, 0], [1, 1, 2, 2, 3, 3]), [1, 3], global_capacity=2)   # the capacity ends inside the fresh grains
    assert r["n_global"] == 3 and r["overflow"] == 1 and r["frames"][1][0].tolist() == [1, 1, 2, 2, 3, 3]
    assert r["first_frame"].tolist() == [0, 1] and r["gid"][1].tolist() == [1, 2, 3]


# ---- the recorded sequence -----------------------------------------------------------------------------------------------

def golden():
    def make():
        d = np.load(os.path.join(GOLDEN, "pf_frames_cfg1.npz"))
        frames = d["frames"].astype(np.int32)
        theta = np.stack([d["theta_x"], d["theta_z"]]).astype(np.float32)
        clean0 = lc.relabel_by_first_pixel(frames[0])
        lut = np.zeros(119, np.int32)
        lut[frames[0].reshape(-1)] = clean0.reshape(-1)      # every one of the 118 ids occurs in frame 0
        assert len(np.unique(frames[0])) == 118
        return {"frames": frames, "theta": theta, "truth": lut[frames], "lut": lut, "G": float(d["G"]), "R": float(d["R"])}
    return cached("golden", make)


def golden_angles(tag):
    """tag "clean" or a noise level d of NOISE -> the seven angle maps float32 [7, 2, 501, 501] and min_pixels."""
    g = golden()
    if tag == "clean":
        return cached(("angles", tag), lambda: np.ascontiguousarray(np.stack([g["theta"][:, f - 1] for f in g["frames"]]))), 1
    seed0 = NOISE[tag][0]
    return cached(("angles", tag), lambda: np.stack([lc.noisy(f, g["theta"], tag, seed0 + 10 * t)[1] for t, f in enumerate(g["frames"])])), 8


def golden_labelled(tag, cap):
    """Every frame labelled on its own by the restatement of the labelling -> (labels [7, 501, 501], n_local, means
    [7, 2, cap] or None, the per-frame status).  tag "ids": the recorded ids; else golden_angles' maps at tol 1e-3."""
    def make():
        g = golden()
        if tag == "ids":
            rs = [lc.label(ids=f) for f in g["frames"]]
        else:
            angles, mp = golden_angles(tag)
            rs = [lc.label(angles=a, tol=1e-3, min_pixels=mp) for a in angles]
        means = None
        if tag != "ids":
            means = np.zeros((7, 2, cap), np.float32)
            for t, r in enumerate(rs):
                means[t, :, :r["n_grain"]] = r["mean_angles"]
        return np.stack([r["image"] for r in rs]), [r["n_grain"] for r in rs], means, [r["status"] for r in rs]
    return cached(("labelled", tag, cap), make)


def golden_linked(tag, cap=128):
    labels, n_local, means, _ = golden_labelled(tag, cap)
    return restated(("golden", tag, cap), labels=labels, n_local=n_local, means=means, local_capacity=cap)


def test_the_recorded_sequence_clean():
    g = golden()
    labels, n_local, _, _ = golden_labelled("ids", 128)
    assert n_local == [118, 118, 118, 118, 117, 111, 100]
    assert not np.array_equal(labels[4], g["truth"][4])                  # (labelling each frame on its own does not give the ids)
    r = golden_linked("ids")
    print(r["candidates"], [words(r, t) for t in range(7)])
    assert np.array_equal(r["frames"], g["truth"])                       # every pixel of all seven frames
    assert [s["n_gone"] for s in r["status"][1:]] == GONE and r["candidates"] == CANDIDATES
    assert all(s["n_fresh"] == 0 == s["n_split"] and s["n_matched"] == s["n_local"] for s in r["status"][1:])
    assert r["n_global"] == 118 and r["overflow"] == 0 and r["first_frame"][:118].tolist() == [0] * 118
    present = [np.unique(f) for f in g["truth"]]
    assert all(r["last_frame"][k - 1] == max(t for t in range(7) if k in present[t]) for k in range(1, 119))


@pytest.mark.parametrize("d", sorted(NOISE))
def test_the_recorded_sequence_under_noise(d):
    g = golden()
    r = golden_linked(d)
    differing = [int((r["frames"][t] != g["truth"][t]).sum()) for t in range(7)]
    print(d, differing, r["candidates"])
    assert r["n_global"] == 118 and all(s["n_fresh"] == 0 == s["n_split"] for s in r["status"])
    assert differing == NOISE[d][1]
    first = np.array([np.nonzero(g["truth"][0].reshape(-1) == k + 1)[0][0] for k in range(118)])
    want = g["theta"][:, g["frames"][0].reshape(-1)[first] - 1]
    assert np.abs(r["theta"][:, :118].astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -24


def test_the_relabelled_sequence_gives_the_recorded_training_table():
    """The restated frames through the restated tracker (tests/trackcheck.py): the pairs and counts of DESIGN 8m's table."""
    r = golden_linked("ids")
    frames = list(r["frames"])
    u = vu.vectorize(frames, [118] * 7, boundary="periodic", grid="points", joint_capacity=None)
    k = tc.track(u, 118, "periodic", patch_pixels=501 * 501, extra_volume=None, shape=frames[0].shape)
    assert k["valid"] == [True] * 6 + [False] and k["pairs"] == [(t, t + 1) for t in range(5)]
    for t, (matched, n_joint, l0, l1, lu, gone) in enumerate(TABLE):
        c = k["counts"][t]
        assert (c["n_matched"], u["status"][t]["n_joint"], c["n_label0"], c["n_label1"], c["n_unlabelled"], c["n_eliminated"]) == \
            (matched, n_joint, l0, l1, lu, gone), t
        assert c["n_ambiguous"] == 0 and c["n_eliminated"] == r["status"][t + 1]["n_gone"]


def test_entry_point_validates_on_the_host():
    lib = _lib.load()
    assert lib.ggnn_version() == 26 == _lib.GGNN_ABI_VERSION and {"ggnn_link_labels", "ggnn_link_workspace_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    assert lib.ggnn_link_labels(None, None) == -1
    wb = lib.ggnn_link_workspace_bytes
    assert wb(0, 8, 0) == 0 and wb(2, 0, 0) == 0 and wb(2, 8, 5) == 0 and wb(2, 8, -1) == 0 and wb(2, 2 ** 31 - 1, 0) == 0 and wb(2 ** 40, 8, 0) == 0
    need = wb(3, 64, 2)
    assert need >= 2 * 64 * 16 * 8 + 3 * 64 * 8 and wb(1, 64, 0) >= 64 * 8 and wb(1, 64, 0) < need
    buf = (ctypes.c_int64 * 64)()                 # (host memory: refused before anything would be launched)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(**kw):
        A = _lib.LinkLabelsArgs(p, p, p, p, p, p, p, p, p, p, p, need, 3, 32, 32, 64, 128, 1, 0.001, 1, 2, 0)
        A.frames_out = None                       # (so that a call that passes every other check still launches nothing)
        for k, v in kw.items():
            setattr(A, k, v)
        return lib.ggnn_link_labels(ctypes.byref(A), None)
    assert call() == -1
    for bad in (dict(labels=None), dict(n_local=None), dict(gid=None), dict(pred=None), dict(first_frame=None), dict(last_frame=None),
                dict(status=None), dict(workspace=None), dict(means=None), dict(theta=None), dict(T=0), dict(nx=2), dict(ny=2),
                dict(nx=1 << 15), dict(ny=1 << 15), dict(local_capacity=0), dict(local_capacity=2 ** 31 - 1), dict(global_capacity=0),
                dict(global_capacity=2 ** 31 - 1), dict(K=-1), dict(K=5), dict(K=0), dict(min_overlap=0), dict(match_tol=-1.0),
                dict(match_tol=float("nan")), dict(boundary=2), dict(n_local=p.value + 4), dict(status=p.value + 4),
                dict(workspace=p.value + 4), dict(labels=p.value + 2), dict(gid=p.value + 2), dict(theta=p.value + 2),
                dict(workspace_bytes=need - 1)):
        assert call(frames_out=p, **bad) == -1, bad


def test_header_binding_and_struct_agree():
    import re
    src = open(os.path.join(ROOT, "include", "ggnn.h")).read()
    for name in ("GGNN_LINK_SLOTS", "GGNN_LINK_RUN", "GGNN_LINK_FRAME_WORDS", "GGNN_LINK_GLOBAL_WORDS"):
        assert f"#define {name} {getattr(_lib, name)}\n" in src, name
    body = re.search(r"typedef struct ggnn_link_labels_args \{(.*?)\} ggnn_link_labels_args;", src, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in _lib.LinkLabelsArgs._fields_]
    assert ctypes.sizeof(_lib.LinkLabelsArgs) == 12 * 8 + 6 * 8 + 4 * 4
    assert vz.LINK_FRAME_WORDS == lk.FRAME_WORDS and len(lk.FRAME_WORDS) == FW and len(lk.GLOBAL_WORDS) == GW


def test_python_entry_points_refuse_what_they_cannot_take():
    host = torch.ones(2, 8, 8, dtype=torch.int32)
    with pytest.raises(_lib.GGNNError, match="device"):
        vz.link_labels(host, [1, 1])
    with pytest.raises(_lib.GGNNError, match="boundary"):
        vz.link_labels(host, [1, 1], boundary="open")
    with pytest.raises(_lib.GGNNError, match="exactly one"):
        vz.label_sequence()
    with pytest.raises(_lib.GGNNError, match="device"):
        vz.label_sequence(ids=host)
    with pytest.raises(_lib.GGNNError, match="equal-shaped"):
        vz.samples_from_orientation_sequence(host, host[:1], 2.0, 0.4, 1e-3)


# ---- GPU: the kernels equal the restatement bit for bit ----------------------------------------------------------------------

GUARD = 64


def guarded_call(labels, n_local, means=None, match_tol=None, min_overlap=1, boundary="periodic", local_capacity=None,
                 global_capacity=None):
    """The entry point itself with GUARD canary words before and after every output and 256 canary bytes round the workspace ->
    dict of the outputs as numpy arrays, "guards" (all canaries intact) and the status words."""
    lib = _lib.load()
    labels = np.ascontiguousarray(labels, np.int32)
    T, ny, nx = labels.shape
    K = 0 if means is None else means.shape[1]
    Lc = (means.shape[2] if K else max(max(n_local), 1)) if local_capacity is None else local_capacity
    Gc = Lc * min(T, 2) if global_capacity is None else global_capacity
    need = lib.ggnn_link_workspace_bytes(T, Lc, K)
    assert need > 0
    sizes = {"frames": T * ny * nx, "gid": T * Lc, "pred": T * Lc, "first_frame": Gc, "last_frame": Gc, "theta": max(K, 1) * Gc}
    out = {k: torch.full((n + 2 * GUARD,), -7, dtype=torch.float32 if k == "theta" else torch.int32, device=DEV) for k, n in sizes.items()}
    n_status = FW * T + GW
    status = torch.full((n_status + 2 * GUARD,), -7, dtype=torch.int64, device=DEV)
    ws = torch.full((need + 2 * 256,), 0x5A, dtype=torch.uint8, device=DEV)
    d_labels = torch.from_numpy(labels).to(DEV)
    d_local = torch.tensor(list(n_local), dtype=torch.int64, device=DEV)
    d_means = None if not K else torch.from_numpy(np.ascontiguousarray(means, np.float32)).to(DEV)
    at = lambda k: out[k][GUARD:].data_ptr()
    A = _lib.LinkLabelsArgs(d_labels.data_ptr(), d_local.data_ptr(), _lib.ptr(d_means), at("frames"), at("gid"), at("pred"), at("first_frame"),
                            at("last_frame"), at("theta") if K else None, status[GUARD:].data_ptr(), ws[256:].data_ptr(), need, T, nx, ny, Lc, Gc,
                            min_overlap, float(np.float32(match_tol or 0)), int(match_tol is not None), K, vz.BOUNDARIES[boundary])
    _lib.check(lib.ggnn_link_labels(ctypes.byref(A), _lib.current_stream()), "ggnn_link_labels")
    torch.cuda.synchronize()
    guards = bool((ws[:256] == 0x5A).all()) and bool((ws[256 + need:] == 0x5A).all())
    guards = guards and bool((status[:GUARD] == -7).all()) and bool((status[GUARD + n_status:] == -7).all())
    got = {}
    for k, n in sizes.items():
        guards = guards and bool((out[k][:GUARD] == -7).all()) and bool((out[k][GUARD + n:] == -7).all())
        got[k] = out[k][GUARD:GUARD + n].cpu().numpy()
    if not K:
        guards = guards and bool((out["theta"] == -7).all())
    got["frames"] = got["frames"].reshape(T, ny, nx)
    got["gid"], got["pred"] = got["gid"].reshape(T, Lc), got["pred"].reshape(T, Lc)
    got["theta"] = got["theta"].reshape(K, Gc) if K else None
    got["guards"], got["words"] = guards, status[GUARD:GUARD + n_status].tolist()
    return got


def assert_equals_restatement(got, r, what):
    print(what, got["words"])
    assert got["guards"], what
    assert got["words"] == lk.status_words(r), (what, got["words"], lk.status_words(r))
    for k in ("frames", "gid", "pred", "first_frame", "last_frame"):
        assert got[k].dtype == np.int32 and got[k].shape == r[k].shape and np.array_equal(got[k], r[k]), (what, k)
    if r["theta"] is None:
        assert got["theta"] is None, what
    else:
        assert got["theta"].shape == r["theta"].shape and np.array_equal(got["theta"].view(np.uint32), r["theta"].view(np.uint32)), what


def both(key, **kw):
    """The device and the restatement on the same keywords."""
    assert_equals_restatement(guarded_call(**kw), restated(key, **kw), key)


def voronoi_stack(ny, nx, boundary, T, seed, K, vanish=True, appear=False):
    """-> keywords of link: T Voronoi frames whose cells drift, one cell that is gone from the last frame on (vanish), one that
    appears in frame 1 and one in the last frame (appear), every frame in a fresh random numbering of its own; K > 0: a mean per
    grain and channel and a match_tol that tells any two grains apart."""
    def make():
        n_side = 1 if min(ny, nx) < 6 else 3 if min(ny, nx) < 24 else 4
        seeds = [list(s) for s in tc.moving_seeds(ny, nx, n_side, T, seed, drift=0.9)]
        if n_side == 1:                               # a 3 x 3 image: two cells side by side
            seeds = [[(1.5, 0.5), (1.5, 2.4)] for _ in range(T)]
        n = len(seeds[0])
        if vanish and T > 1:
            seeds[T - 1][n // 2] = None
        if appear and T > 1:
            for t in range(T):
                seeds[t] = seeds[t] + [None if t < 1 else (ny * 0.3, nx * 0.6), None if t < T - 1 else (ny * 0.7, nx * 0.2)]
        periodic = boundary == "periodic"
        first = lk.first_id(boundary)
        original = np.stack([tc.voronoi(s, ny, nx, periodic=periodic) for s in seeds])
        raster = np.stack([lc.relabel_by_first_pixel(f) + (first - 1) for f in original])
        labels, n_local = lk.renumber(raster, seed + 1, boundary)
        kw = dict(labels=labels, n_local=n_local, boundary=boundary)
        if K:
            rs = np.random.RandomState(seed + 2)
            per_seed = f32(rs.permutation(len(seeds[0]) * K).reshape(K, -1) * 0.03125 + 0.0625)     # any two differ by 1 / 32 at least
            Lc = max(n_local) + 3
            means = np.full((T, K, Lc), np.nan, np.float32)
            for t in range(T):
                ids, at = np.unique(labels[t], return_index=True)
                keep = ids >= first
                means[t][:, ids[keep] - first] = per_seed[:, original[t].reshape(-1)[at[keep]] - 1]
            kw.update(means=means, match_tol=0.01, local_capacity=Lc)
        return kw
    return cached(("voronoi", ny, nx, boundary, T, seed, K, vanish, appear), make)


RUN_SHAPES = [(15, 65), (16, 64), (33, 127), (3, 3)]      # each side of a 64 x 16 tile and of a thread's run of four pixels


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("shape", RUN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_voronoi_stacks_that_drift(shape, boundary):
    for K in (0, 2):
        kw = voronoi_stack(*shape, boundary, 3, 5, K)
        r = restated(("voronoi", shape, boundary, K), **kw)
        if shape != (3, 3):
            assert r["status"][2]["n_gone"] >= 1 and not np.array_equal(kw["labels"][1], r["frames"][1])
        assert r["overflow"] == 0 and r["n_global"] >= kw["n_local"][0]
        both(("voronoi", shape, boundary, K), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 5])
def test_one_frame_and_five(T):
    for boundary in BOUNDARIES:
        kw = voronoi_stack(33, 127, boundary, T, 9, 2, appear=True)
        r = restated(("frames", T, boundary), **kw)
        assert r["n_global"] == kw["n_local"][0] + (2 if T > 1 else 0)
        both(("frames", T, boundary), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_drawn_cases_on_the_device(name):
    both(("hand", name), **HAND[name][0])


def stripes(n, width=2, height=4):
    """Frame 0: n vertical stripes; frame 1: one grain over all of them, and a second one in a last column of its own."""
    row0 = [1 + k for k in range(n) for _ in range(width)] + [n + 1]
    return stack(row0, [1] * (n * width) + [2], height=height), [n + 1, 2]


@pytest.mark.gpu
def test_a_grain_over_sixteen_grains_is_exact_and_over_seventeen_is_counted():
    labels, n_local = stripes(_lib.GGNN_LINK_SLOTS)
    r = restated("sixteen stripes", labels=labels, n_local=n_local)
    assert r["candidates"] == [16] and r["status"][1]["n_gone"] == 15 and r["frames"][1][0].tolist() == [1] * 32 + [17]
    both("sixteen stripes", labels=labels, n_local=n_local)
    labels, n_local = stripes(_lib.GGNN_LINK_SLOTS + 1)
    got = guarded_call(labels, n_local)
    print(got["words"])
    assert got["guards"] and got["words"][FW + lk.FRAME_WORDS.index("n_vote_overflow")] > 0 and got["words"][lk.FRAME_WORDS.index("n_vote_overflow")] == 0
    with pytest.raises(_lib.GGNNError, match="votes"):
        vz.link_labels(torch.from_numpy(labels).to(DEV), n_local)


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_capacities_inside_the_grains(boundary):
    kw = voronoi_stack(33, 127, boundary, 3, 9, 2, appear=True)
    full = restated(("frames", 3, boundary), **kw)
    assert full["n_global"] == kw["n_local"][0] + 2 and full["overflow"] == 0
    # global: the rows end between the two fresh grains; the images are complete
    small = dict(kw, global_capacity=kw["n_local"][0] + 1)
    r = restated(("capacity", "global", boundary), **small)
    assert r["overflow"] == 1 and np.array_equal(r["frames"], full["frames"]) and r["n_global"] == full["n_global"]
    both(("capacity", "global", boundary), **small)
    # local: the rows end two below a frame's ids
    Lc = max(kw["n_local"]) - 2
    small = dict(kw, means=np.ascontiguousarray(kw["means"][:, :, :Lc]), local_capacity=Lc)
    r = restated(("capacity", "local", boundary), **small)
    assert r["overflow"] > 3 and int((r["frames"] == 0).sum()) > 0
    both(("capacity", "local", boundary), **small)
    with pytest.raises(_lib.GGNNError, match="overflow"):
        vz.link_labels(to_dev(kw["labels"]), kw["n_local"], means=to_dev(kw["means"]), match_tol=kw["match_tol"],
                       global_capacity=kw["n_local"][0] + 1, boundary=boundary)


def to_dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.gpu
def test_two_runs_and_a_captured_graph_give_the_same_bits():
    kw = voronoi_stack(33, 127, "periodic", 5, 9, 2, appear=True)
    r = restated(("frames", 5, "periodic"), **kw)
    args = (to_dev(kw["labels"]), torch.tensor(kw["n_local"], device=DEV), to_dev(kw["means"]), kw["match_tol"], 1, "periodic", None, None)
    first, second = vz._link_checked(*args), vz._link_checked(*args)      # (also the warm-up of the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = vz._link_checked(*args)
    for _ in range(2):                                                    # (a replay starts from its own memsets)
        graph.replay()
    torch.cuda.synchronize()
    for k in ("frames", "gid", "pred", "first_frame", "last_frame", "theta", "status"):
        assert torch.equal(first[k], second[k]) and torch.equal(first[k], held[k]), k
    assert held["status"].tolist() == lk.status_words(r) and np.array_equal(held["frames"].cpu().numpy(), r["frames"])
    # the public call: the same results cut to the grains there are, from a device n_local and from a host list
    for n_local in (args[1], kw["n_local"]):
        frames, n_grain, theta, report = vz.link_labels(args[0], n_local, means=args[2], match_tol=kw["match_tol"])
        n = r["n_global"]
        assert n_grain == n == report["n_global"] and report["frames"] == r["status"] and torch.equal(frames, held["frames"])
        assert np.array_equal(theta.cpu().numpy().view(np.uint32), r["theta"][:, :n].view(np.uint32))
        assert report["first_frame"].tolist() == r["first_frame"][:n].tolist() and report["last_frame"].tolist() == r["last_frame"][:n].tolist()
        assert torch.equal(report["gid"], held["gid"]) and torch.equal(report["pred"], held["pred"])


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


@pytest.mark.gpu
def test_label_sequence_on_the_recorded_frames_in_ids_mode(monkeypatch):
    g = golden()
    cap = 65536                                                           # the default room per frame at min_pixels 1
    labels, n_local, _, label_status = golden_labelled("ids", 128)
    r = restated(("golden", "ids", cap), labels=labels, n_local=n_local, local_capacity=cap)
    ids = torch.from_numpy(g["frames"]).to(DEV)
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        counted = Counted(m)
        frames, n_grain, theta, report = vz.label_sequence(ids=ids)
        assert counted.n == 1                                             # one read-back
    assert n_grain == 118 and theta is None and report["label"] == label_status and report["frames"] == r["status"]
    assert np.array_equal(frames.cpu().numpy(), r["frames"]) and np.array_equal(r["frames"], g["truth"])
    assert np.array_equal(report["gid"].cpu().numpy(), r["gid"]) and np.array_equal(report["pred"].cpu().numpy(), r["pred"])
    assert report["last_frame"].tolist() == r["last_frame"][:118].tolist() and [s["n_gone"] for s in report["frames"][1:]] == GONE


@pytest.mark.gpu
def test_label_sequence_on_noisy_angle_maps(monkeypatch):
    g = golden()
    angles, mp = golden_angles(0.04)
    cap = min(501 * 501 // mp + 2, 65536)
    labels, n_local, means, label_status = golden_labelled(0.04, cap)
    r = restated(("golden", 0.04, cap), labels=labels, n_local=n_local, means=means, local_capacity=cap)
    dev = torch.from_numpy(angles).to(DEV)
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        counted = Counted(m)
        frames, n_grain, theta, report = vz.label_sequence(angles=dev, tol=1e-3, min_pixels=mp)
        assert counted.n == 1
    assert n_grain == 118 and report["label"] == label_status and report["frames"] == r["status"]
    assert np.array_equal(frames.cpu().numpy(), r["frames"])
    assert [int((r["frames"][t] != g["truth"][t]).sum()) for t in range(7)] == NOISE[0.04][1]
    assert theta.shape == (2, 118) and np.array_equal(theta.cpu().numpy().view(np.uint32), r["theta"][:, :118].view(np.uint32))
    assert np.array_equal(report["gid"].cpu().numpy(), r["gid"]) and np.array_equal(report["pred"].cpu().numpy(), r["pred"])


def assert_same_sample(a, b):
    for da, db in zip(a, b):
        assert da.keys() == db.keys()
        for k in da:
            assert da[k].dtype == db[k].dtype and torch.equal(da[k], db[k]), k


@pytest.mark.gpu
def test_samples_from_an_orientation_sequence_and_one_batch():
    from graingraphnn_amd import training
    g = golden()
    angles, mp = golden_angles("clean")
    cap = 65536
    labels, n_local, means, _ = golden_labelled("clean", cap)
    r = restated(("golden", "clean", cap), labels=labels, n_local=n_local, means=means, local_capacity=cap)
    assert np.array_equal(r["frames"], g["truth"]) and r["n_global"] == 118
    dev = torch.from_numpy(angles).to(DEV)
    kw = dict(patch_pixels=501 * 501, grid="points")
    samples, report, frames = vz.samples_from_orientation_sequence(dev[:, 0], dev[:, 1], g["G"], g["R"], 1e-3, min_pixels=mp, **kw)
    assert np.array_equal(frames.cpu().numpy(), r["frames"])
    seq = report["sequence"]
    assert np.array_equal(np.stack([seq["theta_x"], seq["theta_z"]]).view(np.uint32), r["theta"][:, :118].view(np.uint32))
    want, want_report = vz.frames_to_samples(to_dev(r["frames"]), r["theta"][0, :118], r["theta"][1, :118], g["G"], g["R"], **kw)
    assert report["pairs"] == want_report["pairs"] == [(t, t + 1) for t in range(5)] and report["counts"] == want_report["counts"]
    assert len(samples) == len(want) == 5
    for t, (a, b) in enumerate(zip(samples, want)):
        assert_same_sample(a, b)
        c = report["counts"][t]
        assert (c["n_matched"], a[0]["joint"].size(0), c["n_label0"], c["n_label1"], c["n_unlabelled"], c["n_eliminated"]) == TABLE[t], t
    ds = training.DeviceDataset(samples, 2)
    db = training.DeviceBatches(ds)
    ds.set_order(np.arange(5))
    db.next()
    for i, sl in zip(ds.batch_ids(0), ds.slices(0)):
        y, mask = samples[i][3], samples[i][4]
        for nt in ("grain", "joint"):
            a, b = sl[nt]
            assert torch.equal(db.y_dict[nt][a:b], y[nt]) and torch.equal(db.mask[nt][a:b].reshape(-1, 1), mask[nt]), (i, nt)
        a, b = sl["grain"]
        assert torch.equal(db.y_dict["grain_event"][a:b], y["grain_event"]), i
