"""The rule of include/ggnn.h's ggnn_label_orientations, restated in numpy: a map of unit quaternions -> the links under
crystal symmetry, the grain-ID image by tests/labelcheck.py's stages, and the per-grain mean orientation.  Every float32
operation is one numpy float32 operation in the header's order (numpy neither contracts nor reassociates), the mean's
normalisation is float64: the device's bits.  Beside it, in float64: the disorientation by brute force over the 24 operators,
and the seeded map recipe of the tests."""
import numpy as np

import labelcheck as lc
import trackcheck as tk

H = np.float32(0.70710678)
_h, _o = float(H), 0.5
OPS = np.array([(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1),
                (_h, _h, 0, 0), (_h, -_h, 0, 0), (_h, 0, _h, 0), (_h, 0, -_h, 0), (_h, 0, 0, _h), (_h, 0, 0, -_h),
                (0, _h, _h, 0), (0, _h, -_h, 0), (0, _h, 0, _h), (0, _h, 0, -_h), (0, 0, _h, _h), (0, 0, _h, -_h),
                (_o, _o, _o, _o), (_o, _o, _o, -_o), (_o, _o, -_o, _o), (_o, _o, -_o, -_o),
                (_o, -_o, _o, _o), (_o, -_o, _o, -_o), (_o, -_o, -_o, _o), (_o, -_o, -_o, -_o)], np.float32)   # s_0 .. s_23 (w, x, y, z)
SCALE = np.float32(16777216.0)
NORM_TOL = np.float32(1e-3)


def cos_half(tol):
    """The one number formed on the host."""
    return np.float32(np.cos(np.float64(tol) / 2))


def qmul(p, q):
    """p (x) q on arrays [4, ...] in their own dtype: four products a component, combined left to right."""
    pw, px, py, pz = p
    qw, qx, qy, qz = q
    return np.stack([((pw * qw - px * qx) - py * qy) - pz * qz, ((pw * qx + px * qw) + py * qz) - pz * qy,
                     ((pw * qy - px * qz) + py * qw) + pz * qx, ((pw * qz + px * qy) - py * qx) + pz * qw])


def conj(q):
    return np.stack([q[0], -q[1], -q[2], -q[3]])


def validity(quats, valid=None):
    q = np.asarray(quats, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        n = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
        ok = np.abs(n - np.float32(1)) <= NORM_TOL
    if valid is not None:
        ok = ok & (np.asarray(valid) != 0)
    return ok


def alike(a, b, symmetry):
    """W float32 [...]: cos of half the disorientation of a and b [4, ...] by the header's closed form."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = qmul(conj(a), b)
        if symmetry == "none":
            return np.abs(r[0])
        m = -np.sort(-np.abs(r), axis=0)                                  # m1 >= m2 >= m3 >= m4
        s12 = m[0] + m[1]
        return np.maximum(m[0], np.maximum(s12 * H, np.float32(0.5) * (s12 + (m[2] + m[3]))))


def links(quats, ok, cos_half_tol, symmetry, periodic):
    q = np.asarray(quats, np.float32)

    def pair(axis):
        with np.errstate(invalid="ignore"):
            out = ok & np.roll(ok, -1, axis) & (alike(q, np.roll(q, -1, axis + 1), symmetry) >= np.float32(cos_half_tol))
        if not periodic:
            if axis == 1:
                out[:, -1] = False
            else:
                out[-1, :] = False
        return out
    return pair(1), pair(0)


def aligned(q_root, q, symmetry):
    """a float32 [4, n]: every q [4, n] as its equivalent nearest q_root [4, n], by the header's rule."""
    ops = OPS if symmetry == "cubic" else OPS[:1]
    r = qmul(conj(q_root), q)
    c = np.stack([qmul(r, np.broadcast_to(s[:, None], r.shape))[0] for s in ops])      # [n_ops, n]
    best = np.argmax(np.abs(c), 0)                                                     # the first of the largest
    cb = c[best, np.arange(c.shape[1])]
    a = qmul(q, np.ascontiguousarray(ops[best].T))
    return np.where(cb < 0, -a, a).astype(np.float32)


def label(quats, tol, valid=None, min_pixels=1, max_sweeps=64, boundary="periodic", grain_capacity=None, symmetry="cubic"):
    """-> dict: image int32 [ny, nx], n_grain, mean_quats float32 [4, min(n_grain, capacity)], status (labelcheck.STATUS), and
    `root`, `state`, `right`, `down` for the tests that look inside."""
    assert boundary in ("periodic", "noflux") and symmetry in ("cubic", "none") and 0 < tol < np.pi / 2
    periodic = boundary == "periodic"
    quats = np.asarray(quats, np.float32)
    _, ny, nx = quats.shape
    ok = validity(quats, valid)
    right, down = links(quats, ok, cos_half(tol), symmetry, periodic)
    root = lc.components(right, down)
    flat = root.reshape(-1)
    size = np.bincount(flat[ok.reshape(-1)], minlength=ny * nx)
    is_root = ok & (root == np.arange(ny * nx).reshape(ny, nx))
    closed = ok & (size[flat].reshape(ny, nx) >= min_pixels)
    grain_roots = np.nonzero((is_root & closed).reshape(-1))[0]
    speck_roots = np.nonzero((is_root & ~closed).reshape(-1))[0]
    state = np.where(closed, root, -1).astype(np.int64)
    n_sweeps = 0
    for _ in range(max_sweeps):
        state, assigned = lc.sweep(state, periodic)
        if not assigned:
            break
        n_sweeps += 1
    first = 1 if periodic else 2
    rank = np.full(ny * nx + 1, -first, np.int64)
    rank[grain_roots] = np.arange(len(grain_roots))
    image = (rank[state.reshape(-1)] + first).astype(np.int32).reshape(ny, nx)
    n_grain = len(grain_roots) + (0 if periodic else 1)
    cap = ny * nx // min_pixels + 2 if grain_capacity is None else int(grain_capacity)
    # the means: over the ORIGINAL components, exact int64 sums of the aligned quaternions, normalised in float64
    qf = quats.reshape(4, -1)
    kept = np.nonzero(closed.reshape(-1))[0]
    S = np.zeros((4, ny * nx), np.int64)
    if len(kept):
        a = aligned(qf[:, flat[kept]], qf[:, kept], symmetry)
        Q = np.rint(a * SCALE).astype(np.int64)
        for k in range(4):
            np.add.at(S[k], flat[kept], Q[k])
    d = S[:, grain_roots].astype(np.float64)
    n2 = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(n2 == 0, qf[:, grain_roots], (d / np.sqrt(n2)).astype(np.float32)).astype(np.float32)
    means = np.zeros((4, min(n_grain, cap)), np.float32)
    if not periodic and cap >= 1:
        means[0, 0] = 1
    g = np.arange(len(grain_roots)) + (first - 1)
    means[:, g[g < cap]] = m[:, g < cap]
    status = dict(n_components=int(is_root.sum()), n_specks=len(speck_roots), n_speck_pixels=int(size[speck_roots].sum()),
                  n_invalid_in=int((~ok).sum()), n_grains=len(grain_roots), n_sweeps=n_sweeps, n_unfilled=int((state < 0).sum()),
                  overflow=int(n_grain > cap), n_bound_hits=0)
    return {"image": image, "n_grain": n_grain, "mean_quats": means, "status": status, "root": root, "state": state,
            "right": right, "down": down}


# ---- float64: the group by brute force, and the recipe --------------------------------------------------------------------

def ops64():
    """The 24 operators with their irrational entries exact to float64."""
    o = OPS.astype(np.float64)
    o[np.abs(np.abs(o) - float(H)) < 1e-6] = np.sign(o[np.abs(np.abs(o) - float(H)) < 1e-6]) * np.sqrt(0.5)
    return o


def brute_w(r, ops=None):
    """max_i |w(r (x) s_i)| in float64 for r [4, n]."""
    ops = ops64() if ops is None else ops
    return np.max(np.abs(np.stack([qmul(r, np.broadcast_to(s[:, None], r.shape))[0] for s in ops])), 0)


def disorientation(a, b, symmetry="cubic"):
    """The disorientation angle in radians of a and b [4, n] (float64, by brute force)."""
    r = qmul(conj(np.asarray(a, np.float64)), np.asarray(b, np.float64))
    r = r / np.sqrt((r * r).sum(0))
    w = brute_w(r) if symmetry == "cubic" else np.abs(r[0])
    return 2 * np.arccos(np.minimum(w, 1.0))


def random_quats(rs, n):
    q = rs.standard_normal((4, n))
    return q / np.sqrt((q * q).sum(0))


def axis_angle(axis, angle):
    """Unit quaternions float64 [4, n] of rotations by angle [n] (radians) about axis [3, n]."""
    axis, angle = np.asarray(axis, np.float64).reshape(3, -1), np.asarray(angle, np.float64).reshape(-1)
    axis = axis / np.sqrt((axis * axis).sum(0))
    return np.concatenate([np.cos(angle / 2)[None], axis * np.sin(angle / 2)])


def bunge_from_quats(q):
    """Bunge angles (phi1, Phi, phi2) in radians whose quaternion Rz(phi1) Rx(Phi) Rz(phi2) is q [4, ...] (float64)."""
    plus, minus = np.arctan2(q[3], q[0]), np.arctan2(q[2], q[1])          # (phi1 + phi2) / 2, (phi1 - phi2) / 2
    return plus + minus, 2 * np.arctan2(np.hypot(q[1], q[2]), np.hypot(q[0], q[3])), plus - minus


def in_variants(q, rs):
    """q [4, n] float64 -> float32: every column times a random one of the 24 operators and a random sign."""
    n = q.shape[1]
    s = np.ascontiguousarray(ops64()[rs.randint(0, 24, n)].T)
    return (qmul(q, s) * rs.choice([-1.0, 1.0], n)).astype(np.float32)


def recipe(ny, nx, boundary, seed, n_cells=None, seeds=None, cell_quats=None):
    """The map recipe -> dict: cells int32 [ny, nx] (ids from 1), cell_quats float64 [4, n] (every pair more than 5 degrees
    apart in cubic disorientation), quats float32 [4, ny, nx]: cell (x) noise (at most 0.3 degrees about a random axis) (x) a
    random operator, times a random sign."""
    rs = np.random.RandomState(seed)
    n = n_cells or max(2, ny * nx // 110)
    if seeds is None:
        seeds = [(rs.uniform(0, ny), rs.uniform(0, nx)) for _ in range(n)]
    n = len(seeds)
    cells = tk.voronoi(seeds, ny, nx, periodic=boundary == "periodic")
    if cell_quats is None:
        cell_quats = random_quats(rs, n)
        for i in range(n):
            while i and disorientation(cell_quats[:, :i], np.repeat(cell_quats[:, i:i + 1], i, 1)).min() <= np.deg2rad(5.0):
                cell_quats[:, i] = random_quats(rs, 1)[:, 0]
    N = ny * nx
    noise = axis_angle(rs.standard_normal((3, N)), rs.uniform(0, np.deg2rad(0.3), N))
    q = qmul(cell_quats[:, cells.reshape(-1) - 1], noise)
    quats = in_variants(q, rs)
    return {"cells": cells, "cell_quats": cell_quats, "quats": np.ascontiguousarray(quats.reshape(4, ny, nx))}


def link_margin(r, tol, symmetry="cubic"):
    """The smallest distance in radians between a neighbour pair's float64 disorientation and tol, over the pairs of two valid
    pixels of the restated map r (from `label`, with `quats` and `periodic` added by the caller)."""
    q, out = r["quats"].astype(np.float64), np.inf
    ok = validity(r["quats"], r.get("valid"))
    for axis in (1, 0):
        both = ok & np.roll(ok, -1, axis)
        if not r["periodic"]:
            both[(slice(None), -1) if axis == 1 else (-1, slice(None))] = False
        with np.errstate(invalid="ignore"):
            ang = disorientation(q.reshape(4, -1), np.roll(q, -1, axis + 1).reshape(4, -1), symmetry).reshape(both.shape)
        if both.any():
            out = min(out, float(np.abs(ang[both] - tol).min()))
    return out
