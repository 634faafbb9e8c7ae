"""Pinch windows read as necks (GGNN_PINCH_NECK of the _pinch_traj entry points, include/ggnn.h; vectorize's pinch="neck"),
restated on top of tests/vectorcheck.py, tests/vectorcheck_noflux.py, tests/vectorcheck_union.py and tests/tracecheck.py without
editing them: the definition the kernels are held to bit for bit.

  pinch window   a window with three distinct valid ids whose repeated id sits on a diagonal: [a b; c a] (TL == BR) or
                 [b a; a c] (TR == BL).  Grain a runs through the pixel corner as a neck one pixel wide; b and c do not meet.
  "junction"     the rule of those files: the window carries the key {a, b, c}.
  "neck"         the window carries NO key.  Valid ids, the periodic wrap, the no-flux outside-reads-as-id-1 convention,
                 quadruple windows and the two-id checkerboard [a b; b a] are unchanged.
Every part of the rule reads one predicate, `window_keys`, so everything follows from swapping it: a pinch window is no
candidate, no carrier in the representative test, not in m, Sx, Sy, not counted as merged, owns nothing and is owned by nobody
in the trace rule, and a walk that reaches it finds a vertex without a key that holds both grains, with exactly two a | b cracks,
and leaves by the other.  `neck()` swaps the predicate in the three modules that hold a reference to it and puts it back.

  n_pinch_windows   the pinch windows of an image, each counted once, by brute force over every window of the mode's range."""
import contextlib

import numpy as np

import tracecheck as tc
import vectorcheck as vc
import vectorcheck_noflux as vn
import vectorcheck_union as vu

PINCHES = ("junction", "neck")
_junction_keys = vc.window_keys


def is_pinch(tl, tr, bl, br, n_grain):
    keys, quad = _junction_keys(tl, tr, bl, br, n_grain)
    return len(keys) == 1 and not quad and (tl == br or tr == bl)


def window_keys(tl, tr, bl, br, n_grain):
    """vectorcheck.window_keys under "neck"."""
    if is_pinch(tl, tr, bl, br, n_grain):
        return [], False
    return _junction_keys(tl, tr, bl, br, n_grain)


@contextlib.contextmanager
def neck(pinch="neck"):
    """The restatements read pinch windows as necks inside the block ("junction": they are left as they are)."""
    if pinch not in PINCHES:
        raise ValueError(f"pinch must be 'junction' or 'neck', got {pinch!r}")
    modules = (vc, vn, tc) if pinch == "neck" else ()
    before = [m.window_keys for m in modules]
    for m in modules:
        m.window_keys = window_keys
    try:
        yield
    finally:
        for m, f in zip(modules, before):
            m.window_keys = f


def pinch_windows(image, n_grain, boundary="periodic"):
    """[(y, x)] of the pinch windows of an image in raster order, by brute force."""
    W = tc.Windows(image, n_grain, 0, boundary)
    if W.periodic:
        tl, tr, first = W.img, np.roll(W.img, -1, 1), 0
        bl, br = np.roll(W.img, -1, 0), np.roll(np.roll(W.img, -1, 0), -1, 1)
    else:
        tl, tr, bl, br, first = W.img[:-1, :-1], W.img[:-1, 1:], W.img[1:, :-1], W.img[1:, 1:], -1
    # every window is looked at; python judges the ones with an equal diagonal between two other pixels
    diagonal = ((tl == br) & (tr != tl) & (bl != tl)) | ((tr == bl) & (tl != tr) & (br != tr))
    return [(int(i) + first, int(k) + first) for i, k in zip(*np.nonzero(diagonal))
            if is_pinch(int(tl[i, k]), int(tr[i, k]), int(bl[i, k]), int(br[i, k]), W.n_grain)]


def vectorize(image, n_grain, grid="cells", merge_radius=2, joint_capacity=None, boundary="periodic", links="unique",
              max_trace=None, pinch="neck"):
    """tests/vectorcheck.py's, tests/vectorcheck_noflux.py's or (links="trace") tests/tracecheck.py's dict under `pinch`, with
    n_pinch_windows beside it (not in the status: the status keeps its seven words)."""
    with neck(pinch):
        if links == "trace":
            v = tc.vectorize(image, n_grain, grid, merge_radius, joint_capacity, boundary, max_trace)
        else:
            one = vc.vectorize if boundary == "periodic" else vn.vectorize
            v = one(image, n_grain, grid, merge_radius=merge_radius, joint_capacity=joint_capacity)
    v["n_pinch_windows"] = len(pinch_windows(image, n_grain, boundary))
    return v


def vectorize_union(images, n_grains, grid="cells", merge_radius=2, joint_capacity=None, boundary="periodic", links="unique",
                    max_trace=None, pinch="neck"):
    """tests/vectorcheck_union.py's or (links="trace") tests/tracecheck.py's union dict under `pinch`, with n_pinch_windows, a
    list of one count per image."""
    with neck(pinch):
        if links == "trace":
            u = tc.vectorize_union(images, n_grains, grid, merge_radius, joint_capacity, boundary, max_trace)
        else:
            u = vu.vectorize(images, n_grains, grid, merge_radius, joint_capacity, boundary)
    u["n_pinch_windows"] = [len(pinch_windows(i, n, boundary)) for i, n in zip(images, n_grains)]
    return u


def is_valid(status, boundary="periodic"):
    return tc.is_valid(status, boundary)
