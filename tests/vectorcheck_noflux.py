"""The junction graph of a NO-FLUX grain-ID image, restated in numpy: the GGNN_BC_NOFLUX mode of ggnn_image_junctions
(csrc/vectorize.hip, include/ggnn.h) is held to this bit for bit.  The periodic rule is tests/vectorcheck.py's; this one
shares its keys, its pairs and its status words and differs where the image has walls.

The rule, exact in integers up to the position:
  image      int32 [ny, nx], NOT periodic, pixel p = grain p - 1; grain 0 (id 1) is the boundary grain that wraps the
             image: valid ids inside are [2, n_grain]; nx, ny > 2 R
  window     (y, x) for y in [-1, ny - 1], x in [-1, nx - 1] = the pixels TL (y, x), TR (y, x + 1), BL (y + 1, x),
             BR (y + 1, x + 1); a pixel OUTSIDE the image reads as id 1; raster index (y + 1)(nx + 1) + (x + 1)
  keys       a window with an INSIDE pixel that is 1 or outside [1, n_grain] carries none; three distinct ids: that sorted
             triple; four: {TL, TR, BR} and {TL, BL, BR}.  (A window on a wall holds two outside pixels and a corner
             window three: neither can hold four ids, and a corner window {1, 1, 1, a} holds two and carries nothing.)
  invalid    every inside pixel that is 1 or outside [1, n_grain] is counted once
  offsets    W' lies at offset (dy, dx) = (y' - y, x' - x) from W when |dy|, |dx| <= R: no wrap, the window range clips
  junctions  representatives, merging and numbering as in the periodic rule, with this raster index
  position   x = ((float)xr + off + (float)Sx / (float)m) * pitch as in the periodic rule (xr, yr may be -1); then, for a
             junction whose triple holds grain 0 -- its representative straddles a wall, because only such windows read
             an outside pixel --:
               xr == -1: x = 0.0f     xr == nx - 1: x = 1.0f     yr == -1: y = 0.0f     yr == ny - 1: y = max_y
             and the coordinate no wall has set is clamped to [0, 1] (x) or [0, max_y] (y).  (The clamp acts next to a
             corner only, where the carriers of one key lie on two walls; with it every junction lies in
             [0, 1] x [0, max_y] and the rollout's boundary step finds nothing to move.)
  max_y      ((float)(ny - 2) + 2 off) / ((float)(nx - 2) + 2 off), each operation rounded to float32: ny / nx for
             "cells", (ny - 1) / (nx - 1) for "points", exactly 1 for a square image
  columns    as in the periodic rule; grain 0's pairs (0, a) link the wall junctions along the walls
  status     the same seven words; n_present_grains counts the ids 2 .. n_grain with a pixel; VALID: overflow,
             n_invalid_pixels and n_open_pairs 0 and n_joint == 2 n_present_grains - 2 (Euler's formula on the sphere,
             grain 0 being the outer face)
  corners    corner_grains = the pixels [0, 0], [0, nx - 1], [ny - 1, 0], [ny - 1, nx - 1] (ids, not grains)
Candidates are found by brute force over all windows; representatives by comparing every pair of carriers of a key."""
import numpy as np

from vectorcheck import PAIRS, STATUS, grid_constants, window_keys  # noqa: F401  (STATUS: the tests compare against it)


def max_y_of(nx, ny, grid):
    f = np.float32
    off, _ = grid_constants(nx, grid)
    return f(f(f(ny - 2) + f(f(2) * off)) / f(f(nx - 2) + f(f(2) * off)))


def is_valid(status):
    return (status["overflow"] == 0 and status["n_invalid_pixels"] == 0 and status["n_open_pairs"] == 0
            and status["n_joint"] == 2 * status["n_present_grains"] - 2)


def vectorize(image, n_grain, grid="cells", merge_radius=2, joint_capacity=None):
    """-> dict of xy float32 [n, 2], triples int32 [n, 3], gj / jj int64 [2, 3 n] (n = min(n_joint, joint_capacity)),
    status (dict of ints), quads, corner_grains (tuple of four ints), max_y (float32), windows (the representative
    (yr, xr) of every junction)."""
    img = np.asarray(image).astype(np.int64)
    ny, nx = img.shape
    R = int(merge_radius)
    assert nx > 2 * R and ny > 2 * R and R >= 0
    off, pitch = grid_constants(nx, grid)
    max_y = max_y_of(nx, ny, grid)
    bad = (img < 2) | (img > n_grain)
    pad = np.ones((ny + 2, nx + 2), np.int64)
    pad[1:-1, 1:-1] = np.where(bad, 0, img)          # (0: outside [1, n_grain] for window_keys, whatever the pixel held)
    tl, tr, bl, br = pad[:-1, :-1], pad[:-1, 1:], pad[1:, :-1], pad[1:, 1:]     # window (y, x) at [y + 1, x + 1]
    stack = np.sort(np.stack([tl, tr, bl, br]), axis=0)
    distinct = 1 + (stack[1:] != stack[:-1]).sum(0)
    carriers, quads = {}, []                         # key -> [(y, x)] in raster order
    for i, j in zip(*np.nonzero(distinct >= 3)):
        keys, quad = window_keys(int(tl[i, j]), int(tr[i, j]), int(bl[i, j]), int(br[i, j]), n_grain)
        if quad:
            quads.append(tuple(int(v) - 1 for v in (tl[i, j], tr[i, j], bl[i, j], br[i, j])))
        for k in keys:
            carriers.setdefault(k, []).append((int(i) - 1, int(j) - 1))
    raster = lambda y, x: (y + 1) * (nx + 1) + (x + 1)
    joints, merged = [], 0                           # (raster index, key, Sx, Sy, m, yr, xr)
    for key, ws in carriers.items():
        for (y, x) in ws:
            near = [(raster(y2, x2), y2 - y, x2 - x) for (y2, x2) in ws if abs(y2 - y) <= R and abs(x2 - x) <= R]
            if any(r < raster(y, x) for r, _, _ in near):
                merged += 1
                continue
            joints.append((raster(y, x), key, sum(dx for _, _, dx in near), sum(dy for _, dy, _ in near), len(near), y, x))
    joints.sort(key=lambda j: (j[0], j[1]))
    n_joint = len(joints)
    cap = n_joint if joint_capacity is None else int(joint_capacity)
    n = min(n_joint, cap)
    f = np.float32
    xy, triples = np.zeros((n, 2), f), np.zeros((n, 3), np.int32)
    for j, (_, key, sx, sy, m, yr, xr) in enumerate(joints[:n]):
        px = f(f(f(xr) + off) + f(f(sx) / f(m))) * pitch
        py = f(f(f(yr) + off) + f(f(sy) / f(m))) * pitch
        if key[0] == 0:
            px = f(0) if xr == -1 else f(1) if xr == nx - 1 else min(max(px, f(0)), f(1))
            py = f(0) if yr == -1 else max_y if yr == ny - 1 else min(max(py, f(0)), max_y)
        xy[j] = px, py
        triples[j] = key
    gj = np.zeros((2, 3 * n), np.int64)
    gj[0], gj[1] = triples.reshape(-1), np.repeat(np.arange(n), 3)
    by_pair = {}
    for j in range(n):
        for a, b in PAIRS:
            by_pair.setdefault((int(triples[j, a]), int(triples[j, b])), []).append(j)
    jj = np.zeros((2, 3 * n), np.int64)
    jj[0] = np.repeat(np.arange(n), 3)
    n_open = 0
    for j in range(n):
        for k, (a, b) in enumerate(PAIRS):
            others = [o for o in by_pair[(int(triples[j, a]), int(triples[j, b]))] if o != j]
            jj[1, 3 * j + k] = others[0] if len(others) == 1 else -1
            n_open += len(others) != 1
    status = {"n_joint": n_joint, "n_quad_windows": len(quads), "n_merged_windows": merged,
              "n_invalid_pixels": int(bad.sum()), "n_open_pairs": n_open,
              "n_present_grains": int(len(np.unique(img[~bad]))), "overflow": int(n_joint > cap)}
    return {"xy": xy, "triples": triples, "gj": gj, "jj": jj, "status": status, "quads": quads,
            "corner_grains": tuple(int(img[y, x]) for y, x in ((0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1))),
            "max_y": max_y, "windows": [(j[5], j[6]) for j in joints[:n]]}
