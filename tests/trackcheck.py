"""Training targets from a recorded sequence of grain-ID images (ggnn_track_junctions / ggnn_track_targets, include/ggnn.h;
vectorize.track_frames / frames_to_samples), restated in numpy on the union that tests/vectorcheck_union.py restates: the
definition the kernels are held to bit for bit.

The frames are the T images of one union, n_grain grains each, with stable ids: local grain g is the same grain in every frame.
  valid     frame t is valid when its status is (vectorcheck.is_valid; no-flux: n_joint == 2 n_present_grains - 2); the pair
            (t, t + 1) is EMITTED when both frames are
  match     junction j of frame t matches junction k of frame t + 1 when the pair is emitted, their local triples are equal and
            that triple occurs exactly once in either frame: next[j] = k, prev[k] = j (union indices), otherwise -1; a junction
            of frame t whose triple occurs more than once in frame t or in frame t + 1 is counted in n_ambiguous of the pair
  y_joint   matched: float32(5.0 * d), d = float64(xy[k]) - float64(xy[j]), periodic: d - 1 if d > 0.5, d + 1 if d < -0.5;
            mask 1; unmatched: 0, mask 0.  hist_joint: the same from prev[j] to j, 0 without one
  labels    column s = 3 j + k of the joint->joint list, u = j, v its destination, in a frame whose pair is emitted:
            0  u and v both matched and next[v] among the three destinations of next[u]
            1  u = {a, b, c} and v = {a, b, d} both unmatched, {a, c, d} and {b, c, d} each occur exactly once in frame t + 1,
               and the second is among the destinations of the first
            -1 everything else, and every column of a frame whose pair is not emitted
  y_grain   [0] = float32(20.0 * (float64(c') / pp - float64(c) / pp)) of the pixel counts in frames t, t + 1,
            [1] = float32(20.0 * extra_volume[t + 1]); mask 1 where c != 0 (not for a no-flux boundary grain, local grain 0);
            event 1 where the mask is 1 and c' == 0; all 0 in a frame whose pair is not emitted
  hist_grain [0] = the area expression from frame t - 1 to t when that pair is emitted, [1] = float32(20.0 * extra_volume[t]);
            both 0 for a grain without pixels in frame t (its row of x is zero but for the orientation, span and process
            columns) and for a no-flux boundary grain
Everything is looked up in dicts of triples: no table is walked."""
import numpy as np

COUNTERS = ("n_matched", "n_ambiguous", "n_label0", "n_label1", "n_unlabelled", "n_eliminated")
PAIRS = ((0, 1), (0, 2), (1, 2))


def frame_valid(status, boundary):
    return (status["overflow"] == 0 and status["n_invalid_pixels"] == 0 and status["n_open_pairs"] == 0
            and status["n_joint"] == 2 * status["n_present_grains"] - (2 if boundary == "noflux" else 0))


def track(u, n_grain, boundary="periodic", patch_pixels=None, extra_volume=None, shape=None):
    """u: vectorcheck_union.vectorize's dict of the T frames (n_grains = [n_grain] * T).  -> dict of next, prev int64 [n],
    y_joint, hist_joint float32 [n, 2], mask_joint float32 [n], edge_label int64 [3 n], y_grain, hist_grain float32
    [T n_grain, 2], mask_grain float32, grain_event int64 [T n_grain], joint_off (clamped to n), valid [T], pairs, and counts: per
    frame t a dict of COUNTERS for the pair (t, t + 1) (zeros where it is not emitted)."""
    T = len(u["status"])
    n = len(u["triples"])
    off = [min(o, n) for o in u["joint_off"]]
    valid = [frame_valid(s, boundary) for s in u["status"]]
    emitted = [t + 1 < T and valid[t] and valid[t + 1] for t in range(T)]
    frame = np.zeros(n, np.int64)
    where = []                                         # per frame: local triple -> its junctions
    for t in range(T):
        frame[off[t]:off[t + 1]] = t
        d = {}
        for j in range(off[t], off[t + 1]):
            d.setdefault(tuple(int(g) - t * n_grain for g in u["triples"][j]), []).append(j)
        where.append(d)
    local = [tuple(int(g) - int(frame[j]) * n_grain for g in u["triples"][j]) for j in range(n)]
    counts = [dict.fromkeys(COUNTERS, 0) for _ in range(T)]
    nxt, prv = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for j in range(n):
        t = int(frame[j])
        if not emitted[t]:
            continue
        here, there = where[t][local[j]], where[t + 1].get(local[j], [])
        if len(here) == 1 and len(there) == 1:
            nxt[j], prv[there[0]] = there[0], j
            counts[t]["n_matched"] += 1
        if len(here) > 1 or len(there) > 1:
            counts[t]["n_ambiguous"] += 1
    periodic = boundary == "periodic"
    xy = u["xy"].astype(np.float64)

    def step(a, b):
        d = xy[b] - xy[a]
        if periodic:
            d = np.where(d > 0.5, d - 1.0, np.where(d < -0.5, d + 1.0, d))
        return (5.0 * d).astype(np.float32)

    y_joint, hist_joint, mask_joint = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.float32)
    for j in range(n):
        if nxt[j] >= 0:
            y_joint[j], mask_joint[j] = step(j, nxt[j]), 1
        if prv[j] >= 0:
            hist_joint[j] = step(prv[j], j)
    dst = u["jj"][1]
    linked = lambda p, q: q in dst[3 * p:3 * p + 3]
    label = np.full(3 * n, -1, np.int64)
    for j in range(n):
        t = int(frame[j])
        if not emitted[t]:
            continue
        for k, (ia, ib) in enumerate(PAIRS):
            s, v, lab = 3 * j + k, int(dst[3 * j + k]), -1
            if v >= 0 and v != j:
                if nxt[j] >= 0 and nxt[v] >= 0:
                    lab = 0 if linked(nxt[j], nxt[v]) else -1
                elif nxt[j] < 0 and nxt[v] < 0:
                    a, b, c = local[j][ia], local[j][ib], local[j][3 - ia - ib]
                    rest = [g for g in local[v] if g != a and g != b]
                    if len(rest) == 1 and rest[0] != c:
                        p = where[t + 1].get(tuple(sorted((a, c, rest[0]))), [])
                        q = where[t + 1].get(tuple(sorted((b, c, rest[0]))), [])
                        if len(p) == 1 and len(q) == 1 and linked(p[0], q[0]):
                            lab = 1
            label[s] = lab
            counts[t][{0: "n_label0", 1: "n_label1", -1: "n_unlabelled"}[lab]] += 1
    if patch_pixels is None:
        patch_pixels = shape[0] * shape[1]
    pp = np.float64(patch_pixels)
    c = u["counts"].astype(np.float64).reshape(T, n_grain)
    ev = np.zeros((T, n_grain)) if extra_volume is None else np.asarray(extra_volume, np.float64).reshape(T, n_grain)
    y_grain, hist_grain = np.zeros((T, n_grain, 2), np.float32), np.zeros((T, n_grain, 2), np.float32)
    mask_grain, event = np.zeros((T, n_grain), np.float32), np.zeros((T, n_grain), np.int64)
    inner = np.ones(n_grain, bool)
    if not periodic:
        inner[0] = False
    for t in range(T):
        if emitted[t]:
            y_grain[t, :, 0] = (20.0 * (c[t + 1] / pp - c[t] / pp)).astype(np.float32)
            y_grain[t, :, 1] = (20.0 * ev[t + 1]).astype(np.float32)
            mask_grain[t] = (c[t] != 0) & inner
            event[t] = (c[t] != 0) & inner & (c[t + 1] == 0)
            counts[t]["n_eliminated"] = int(event[t].sum())
        if t >= 1 and emitted[t - 1]:
            hist_grain[t, :, 0] = np.where(inner & (c[t] != 0), (20.0 * (c[t] / pp - c[t - 1] / pp)).astype(np.float32), 0)
        hist_grain[t, :, 1] = np.where(inner & (c[t] != 0), (20.0 * ev[t]).astype(np.float32), 0)
    return {"next": nxt, "prev": prv, "y_joint": y_joint, "hist_joint": hist_joint, "mask_joint": mask_joint, "edge_label": label,
            "y_grain": y_grain.reshape(-1, 2), "hist_grain": hist_grain.reshape(-1, 2), "mask_grain": mask_grain.reshape(-1),
            "grain_event": event.reshape(-1), "joint_off": off, "valid": valid,
            "pairs": [(t, t + 1) for t in range(T) if emitted[t]], "counts": counts}


def cut(r, n_grain, t):
    """The (y, mask) of sample t (frames_to_samples' layout) from `track`'s result, and its history columns
    (x_grain[:, 10], x_grain[:, 4], x_joint[:, 6:8])."""
    g0, g1, j0, j1 = t * n_grain, (t + 1) * n_grain, r["joint_off"][t], r["joint_off"][t + 1]
    y = {"grain": r["y_grain"][g0:g1], "joint": r["y_joint"][j0:j1], "edge_event": r["edge_label"][3 * j0:3 * j1],
         "grain_event": r["grain_event"][g0:g1]}
    mask = {"grain": r["mask_grain"][g0:g1].reshape(-1, 1), "joint": r["mask_joint"][j0:j1].reshape(-1, 1)}
    return y, mask, (r["hist_grain"][g0:g1, 0], r["hist_grain"][g0:g1, 1], r["hist_joint"][j0:j1])


# ---- synthetic frames ----------------------------------------------------------------------------------------------------

def voronoi(seeds, ny, nx, periodic=True, first_id=1):
    """The Voronoi image of seeds [(y, x)] in pixels: pixel (y, x) takes the id of the nearest seed (the torus' minimum image
    when periodic; ties go to the lower id), seed i having the id first_id + i.  A seed of None is left out, ids unchanged."""
    yy, xx = np.mgrid[0:ny, 0:nx]
    best, image = np.full((ny, nx), np.inf), np.zeros((ny, nx), np.int32)
    for i, s in enumerate(seeds):
        if s is None:
            continue
        dy, dx = np.abs(yy + 0.5 - s[0]), np.abs(xx + 0.5 - s[1])
        if periodic:
            dy, dx = np.minimum(dy, ny - dy), np.minimum(dx, nx - dx)
        d = dy * dy + dx * dx
        take = d < best
        best[take], image[take] = d[take], first_id + i
    return image


def moving_seeds(ny, nx, n_side=4, T=3, seed=0, drift=0.6):
    """T frames of n_side x n_side jittered lattice seeds that drift a little from frame to frame: [T][(y, x)]."""
    rs = np.random.RandomState(seed)
    base = [((i + 0.5) * ny / n_side + rs.uniform(-0.25, 0.25) * ny / n_side, (k + 0.5) * nx / n_side + rs.uniform(-0.25, 0.25) * nx / n_side)
            for i in range(n_side) for k in range(n_side)]
    frames = [base]
    for _ in range(T - 1):
        frames.append([(y + rs.uniform(-drift, drift), x + rs.uniform(-drift, drift)) for y, x in frames[-1]])
    return frames
