"""Restatement of an in-between layer of a rollout (ggnn_interp_polygons, include/ggnn.h; the reference's --interp_frames,
test.py:494-528) in numpy float32, operation by operation in the device's sequence, then polycheck.restate on the result.

A job is (layer L >= 1, coefficient c in [0, 1]); X_L and X_prev are the junctions of layers L and L - 1 in the global frame
(float32 [n_joint, 2]); the table is layer T's with T = L where c > 0.5, else L - 1; O is the other layer:
    seam   : periodic: O's coordinate to the minimum image of T's: o += (-1 if o - t > 0.5 else (1 if o - t < -0.5 else 0))
    blend  : v = fl(fl(c) * X_L) + fl(fl(1 - c) * X_prev), 1 - c formed in double and rounded once
    wrap   : periodic: v -= floor(v) where v is not in [0, 1) although T's coordinate is (a recorded coordinate outside
             [0, 1) -- the junctions are never wrapped -- keeps the blend where it is: c = 0 and c = 1 are the layers' own)
    snap   : no-flux: the junctions of the boundary grain's row (grain 0, or every non-empty trajectory's first grain) take
             d = [x, 1 - x, y, max_y - y] of the UNCLAMPED blend; the first minimum decides; that coordinate becomes 0, 1, 0
             or max_y
    clamp  : no-flux: every junction to [0, 1] x [0, max_y]
Periodic jobs neither snap nor clamp, and blend along the short way across a wall: the two departures from the reference
script."""
import numpy as np

import polycheck

F = np.float32


def min_image(o, t):
    """periodic_move of o towards t, elementwise in float32 (the device's min_image)."""
    rel = (o - t).astype(F)
    return (o + np.where(rel > F(0.5), F(-1.0), np.where(rel < F(-0.5), F(1.0), F(0.0))).astype(F)).astype(F)


def blend(X_L, X_prev, c, boundary):
    """The junction positions before the walls: seam, blend, wrap.  float32 [n_joint, 2]."""
    xl, xp = np.array(X_L, dtype=F)[:, :2], np.array(X_prev, dtype=F)[:, :2]
    t = xl if c > 0.5 else xp
    if boundary == "periodic":
        if c > 0.5:
            xp = min_image(xp, xl)
        else:
            xl = min_image(xl, xp)
    v = ((F(c) * xl).astype(F) + (F(1.0 - c) * xp).astype(F)).astype(F)
    if boundary == "periodic":
        out = ~((v >= 0) & (v < 1)) & (t >= 0) & (t < 1)
        with np.errstate(invalid="ignore"):
            v[out] = (v[out] - np.floor(v[out])).astype(F)
    return v


def first_minimum(d):
    """torch.argmin's choice among equal minima: the first (a strict < scan, as the device's)."""
    k, m = 0, d[0]
    for i in range(1, len(d)):
        if d[i] < m:
            k, m = i, d[i]
    return k


def positions(rowptr_T, col_T, X_L, X_prev, c, boundary="periodic", max_y=1.0, traj_grain_off=None):
    """The finished positions of a job: what the rows read.  float32 [n_joint, 2]."""
    v = blend(X_L, X_prev, c, boundary)
    if boundary != "noflux":
        return v
    top = np.array([1.0, max_y], dtype=F)
    out = np.minimum(np.maximum(v, F(0.0)), top).astype(F)
    rowptr_T, col_T = np.asarray(rowptr_T, np.int64), np.asarray(col_T, np.int64)
    for g in sorted(polycheck.boundary_grains(len(rowptr_T) - 1, boundary, traj_grain_off)):
        for j in col_T[rowptr_T[g]:rowptr_T[g + 1]]:
            x, y = v[j]
            k = first_minimum([x, F(F(1.0) - x), y, F(top[1] - y)])
            out[j, k >> 1] = (F(0.0), F(1.0), F(0.0), top[1])[k]
    return out


def restate_job(rowptr_T, col_T, X_L, X_prev, c, boundary="periodic", max_y=1.0, traj_grain_off=None, dtype=np.float32):
    """The record of job (L, c): polycheck.restate's dict on the job's positions with layer T's table, plus `positions`."""
    xy = positions(rowptr_T, col_T, X_L, X_prev, c, boundary, max_y, traj_grain_off)
    r = polycheck.restate(rowptr_T, col_T, xy, boundary=boundary, traj_grain_off=traj_grain_off, dtype=dtype)
    r["positions"] = xy
    return r


def crossed_a_wall(X_L, X_prev):
    """Junctions whose two recorded positions differ by more than half the period in a coordinate: the ones the periodic
    blend takes the short way (bool [n_joint])."""
    d = np.abs(np.asarray(X_L, np.float64)[:, :2] - np.asarray(X_prev, np.float64)[:, :2])
    return (d > 0.5).any(axis=1)


def volume_order(layers, interp_frames):
    """test.py's order of `alpha_field_list`: layer 0, then for each later layer its in-between frames and the layer.
    -> list of ('job', L, c) / ('layer', k)."""
    out = []
    for k in layers:
        if k > 0:
            out += [("job", k, (1 + i) / (1 + interp_frames)) for i in range(interp_frames)]
        out.append(("layer", k))
    return out
