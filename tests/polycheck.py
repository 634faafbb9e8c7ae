"""Restatement of the grains' junction polygons (graph.update(), graph_datastruct.py:654-721: `regions`, `region_coors`,
`region_center`) in numpy, in float64 and in float32, and the classification of the grains the two may differ on.

Per grain g with the junctions j_0 .. j_{n-1} of its row of the joint->grain table, in the row's order:
    global  : xy = (x_joint[j, :2] + domain_offset[j]) / domain_factor when domain_factor > 1          (test.py:474)
    unwrap  : periodic: v_i = periodic_move(v_i, v_{i-1}) for i = 1 .. n-1 (min image to the previous MOVED one, :55-72,
              691-692); no-flux: no chaining
    shift   : +1 in a coordinate where any vertex is below -1e-12                                       (:698-704)
    centre  : the mean                                                                                  (:708)
    order   : ascending in counterclock()'s key (:100-116): the angle of v - centre in [0, 2 pi), then its length, then
              the position in the row (sorted() is stable); no-flux: the boundary grain reversed       (:712-716)
    area    : half the sum of cross(v_i - centre, v_next(i) - centre) over the ordered polygon
Rows of 0 or 1 junction are copied as they are (:683), with area 0.

`restate(..., dtype=np.float64)` is that rule with every operation in float64 on the float32 inputs and atan2 / hypot as
the key.  `restate(..., dtype=np.float32)` is the DEVICE's sequence, operation by operation, every one rounded to float32
on its own: the sum of a row runs in the row's order from 0, the centre is sum / n and then + 1 where the vertices were
shifted, the vertices + the shift, d = v - centre, and the key is (quadrant, q, |dx| + |dy|, position) with q = |dy| /
(|dx| + |dy|) in quadrants 0 and 2 and |dx| / (|dx| + |dy|) in 1 and 3 -- the angle's order without atan2 (include/ggnn.h,
ggnn_grain_polygons).  The kernel's joint_sorted, xy_sorted and centre must equal it BIT FOR BIT; its area stays within
`area_bound`.

Where float32 and float64 may differ (classify): a grain's ORDER can differ only where two of its vertices are closer in
angle than the rounding of the keys -- `gap`, the smallest angular gap in float64, tells -- and its START VERTEX where a
vertex sits on the 0 / 2 pi seam -- `seam`, min(angle, 2 pi - angle) over its vertices.
"""
import math

import numpy as np

EPS = -1e-12            # graph_datastruct.py:36, 701
GAP_MIN = 1e-3          # the cyclic sequence is compared for grains whose smallest angular gap is at least this (rad)
SEAM_MIN = 1e-4         # the start vertex where the seam distance exceeds this (rad)
U32 = 2.0 ** -24        # unit roundoff of float32


def table_of(edge_index_jg, n_grain):
    """(rowptr, col) of a joint->grain list [2, E]: the junctions of every grain in the list's order (a stable grouping)."""
    src, dst = np.asarray(edge_index_jg[0], np.int64), np.asarray(edge_index_jg[1], np.int64)
    order = np.argsort(dst, kind="stable")
    rowptr = np.zeros(n_grain + 1, np.int64)
    np.add.at(rowptr, dst + 1, 1)
    return np.cumsum(rowptr), src[order]


def _key64(dx, dy):
    """counterclock(), graph_datastruct.py:100-116."""
    length = math.hypot(dx, dy)
    if length == 0:
        return -math.pi, 0.0
    angle = math.atan2(dy, dx)
    return (2 * math.pi + angle if angle < 0 else angle), length


def _key32(dx, dy):
    f = np.float32
    ax, ay = f(abs(dx)), f(abs(dy))
    den = f(ax + ay)
    if not den > 0:
        return -1, f(0), den
    if dy >= 0:
        return (0, f(ay / den), den) if dx > 0 else (1, f(ax / den), den)
    return (2, f(ay / den), den) if dx < 0 else (3, f(ax / den), den)


def _row(xy, periodic, dtype):
    """One row of >= 2 vertices: (unwrapped and shifted vertices [n, 2], centre [2]) in `dtype`, the device's sequence."""
    f = dtype
    v = np.array(xy, dtype=f)
    n = len(v)
    if periodic:
        for i in range(1, n):
            for c in range(2):
                rel = f(v[i, c] - v[i - 1, c])
                v[i, c] = f(v[i, c] + f(-1.0 if rel > 0.5 else (1.0 if rel < -0.5 else 0.0)))
    centre = np.zeros(2, f)
    for c in range(2):
        s = f(0)
        for i in range(n):
            s = f(s + v[i, c])
        shift = f(0.0) if v[:, c].min() > f(EPS) else f(1.0)
        if f is np.float64:   # the reference: the mean of the shifted vertices
            v[:, c] = v[:, c] + shift
            centre[c] = np.mean(v[:, c])
        else:
            centre[c] = f(f(s / f(n)) + shift)
            v[:, c] = (v[:, c] + shift).astype(f)
    return v, centre


def boundary_grains(n_grain, boundary, traj_grain_off=None):
    """The grains whose order is reversed: none (periodic); grain 0, or every non-empty trajectory's first grain."""
    if boundary != "noflux":
        return set()
    if traj_grain_off is None:
        return {0}
    off = np.asarray(traj_grain_off, np.int64)
    return {int(a) for a, z in zip(off[:-1], off[1:]) if z > a and a < n_grain}


def restate(rowptr, col, x_joint, *, boundary="periodic", domain_factor=1.0, domain_offset=None, traj_grain_off=None,
            dtype=np.float32):
    """-> dict of `joint_sorted` int64 [E], `xy_sorted` dtype [E, 2], `centre` dtype [n, 2], `area` float64 [n] (the exact
    area of the ordered polygon of xy_sorted), `area_terms` float64 [n] (the sum of the absolute values of the halved
    products the area is made of, taken relative to the centre), `sides` [n]."""
    f = dtype
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n_grain, E = len(rowptr) - 1, int(rowptr[-1])
    xy = np.asarray(x_joint, np.float32)[:, :2].astype(f)
    if domain_factor > 1:
        off = np.zeros_like(xy) if domain_offset is None else np.asarray(domain_offset, np.float32).astype(f)
        xy = ((xy + off).astype(f) / f(domain_factor)).astype(f)
    reverse = boundary_grains(n_grain, boundary, traj_grain_off)
    out = {"joint_sorted": np.zeros(E, np.int64), "xy_sorted": np.zeros((E, 2), f), "centre": np.zeros((n_grain, 2), f),
           "area": np.zeros(n_grain), "area_terms": np.zeros(n_grain), "sides": np.diff(rowptr)}
    for g in range(n_grain):
        p0, p1 = int(rowptr[g]), int(rowptr[g + 1])
        js, n = col[p0:p1], p1 - p0
        if n <= 1:
            out["joint_sorted"][p0:p1] = js
            out["xy_sorted"][p0:p1] = xy[js]
            if n == 1:
                out["centre"][g] = xy[js[0]]
            continue
        v, centre = _row(xy[js], boundary == "periodic", f)
        if f is np.float64:
            keys = [_key64(v[i, 0] - centre[0], v[i, 1] - centre[1]) + (i,) for i in range(n)]
        else:
            keys = [_key32(f(v[i, 0] - centre[0]), f(v[i, 1] - centre[1])) + (i,) for i in range(n)]
        order = sorted(range(n), key=lambda i: keys[i])
        if g in reverse:
            order.reverse()
        out["joint_sorted"][p0:p1] = js[order]
        out["xy_sorted"][p0:p1] = v[order]
        out["centre"][g] = centre
        d = v[order].astype(np.float64) - centre.astype(np.float64)
        nx = np.roll(d, -1, axis=0)
        out["area"][g] = 0.5 * float(np.sum(d[:, 0] * nx[:, 1]) - np.sum(d[:, 1] * nx[:, 0]))
        out["area_terms"][g] = 0.5 * float(np.sum(np.abs(d[:, 0] * nx[:, 1])) + np.sum(np.abs(d[:, 1] * nx[:, 0])))
    return out


def area_bound(r):
    """|area32 - area| <= 4 n 2^-24 sum |terms| per grain.  The float32 area is half a sum of 2n products of differences
    d = fl(v - centre): every d carries one rounding (relative 2^-24), every product one more -- (1 + u)^3 - 1 < 3.1 u on
    each term -- and the sum of the n cross terms, in any order, at most (n - 1) u more on the sum of their absolute
    values (a fused multiply-add only removes roundings): (n + 2.1) u sum|terms| <= 4 n u sum|terms| for n >= 2.  The exact
    area does not depend on the point the cross products are taken from."""
    return 4.0 * r["sides"] * U32 * r["area_terms"]


def classify(rowptr, col, x_joint, **kw):
    """Per grain, from the float64 restatement: `gap` = the smallest angular gap between two of its vertices round the
    centre (rad; inf for fewer than 2 vertices) and `seam` = min(angle, 2 pi - angle) over its vertices."""
    r = restate(rowptr, col, x_joint, dtype=np.float64, **kw)
    n_grain = len(r["sides"])
    gap, seam = np.full(n_grain, np.inf), np.full(n_grain, np.inf)
    for g in range(n_grain):
        p0, p1 = int(rowptr[g]), int(rowptr[g + 1])
        if p1 - p0 < 2:
            continue
        d = r["xy_sorted"][p0:p1] - r["centre"][g]
        ang = np.sort(np.array([_key64(x, y)[0] for x, y in d]))
        gap[g] = float(np.min(np.diff(np.concatenate([ang, ang[:1] + 2 * math.pi]))))
        seam[g] = float(np.min(np.minimum(np.abs(ang), 2 * math.pi - ang)))
    return {"gap": gap, "seam": seam, "restated": r}


def rotation_of(a, b):
    """The r with np.roll(b, -r) == a (b is a rotated by r places), or None.  Sequences of distinct ids."""
    a, b = list(a), list(b)
    if len(a) != len(b):
        return None
    if not a:
        return 0
    for r in [i for i, v in enumerate(b) if v == a[0]]:
        if b[r:] + b[:r] == a:
            return r
    return None


def compare_with_reference(got_joint, rowptr, regions, cls):
    """The contract against the reference's `regions` (a list per grain of junction ids, or None for a grain it skipped):
    the cyclic sequence for every grain whose gap is at least GAP_MIN, the start vertex too where the seam distance exceeds
    SEAM_MIN.  -> dict of `excluded` (grains below GAP_MIN), `cyclic_bad`, `start_bad` (lists of grains), `compared`."""
    out = {"excluded": [], "cyclic_bad": [], "start_bad": [], "compared": 0}
    for g, ref in enumerate(regions):
        p0, p1 = int(rowptr[g]), int(rowptr[g + 1])
        if ref is None or p1 - p0 < 2:
            continue
        if cls["gap"][g] < GAP_MIN:
            out["excluded"].append(g)
            continue
        out["compared"] += 1
        r = rotation_of([int(v) for v in ref], [int(v) for v in got_joint[p0:p1]])
        if r is None:
            out["cyclic_bad"].append(g)
        elif r != 0 and cls["seam"][g] > SEAM_MIN:
            out["start_bad"].append(g)
    return out
