"""The labelling rule of include/ggnn.h (ggnn_label_grains), restated by brute force in numpy: an orientation map or a noisy
id image -> a grain-ID image, the number of grains, the per-grain mean angles and the status words.  No kernel, no scipy:
components by hooking every link's larger root under the smaller one and jumping pointers until nothing moves, the cleanup
as whole-image Jacobi sweeps, the numbering by sorting the roots, the means as exact int64 sums."""
import numpy as np

STATUS = ("n_components", "n_specks", "n_speck_pixels", "n_invalid_in", "n_grains", "n_sweeps", "n_unfilled", "overflow",
          "n_bound_hits")
SCALE = np.float32(16777216.0)   # 2^24: the fixed point of the angle sums
MAX_ANGLE = np.float32(8.0)


def validity(ids=None, angles=None, valid=None):
    """bool [ny, nx]: the VALID pixels of either input form."""
    if ids is not None:
        ok = np.asarray(ids) >= 1
    else:
        a = np.asarray(angles, np.float32)
        with np.errstate(invalid="ignore"):
            ok = np.all(np.isfinite(a) & (np.abs(a) <= MAX_ANGLE), axis=0)
    if valid is not None:
        ok = ok & (np.asarray(valid) != 0)
    return ok


def links(ids, angles, tol, ok, periodic):
    """(right, down) bool [ny, nx]: pixel (y, x) is LINKED to (y, x + 1) / (y + 1, x), wrapped when periodic; no link leaves a
    no-flux image."""
    def pair(axis):
        ok2 = np.roll(ok, -1, axis)
        if ids is not None:
            same = np.asarray(ids) == np.roll(np.asarray(ids), -1, axis)
        else:
            a = np.asarray(angles, np.float32)
            with np.errstate(invalid="ignore", over="ignore"):
                same = np.all(np.abs(a - np.roll(a, -1, axis + 1)) <= np.float32(tol), axis=0)   # one fp32 subtraction a channel
        out = ok & ok2 & same
        if not periodic:
            if axis == 1:
                out[:, -1] = False
            else:
                out[-1, :] = False
        return out
    return pair(1), pair(0)


def components(right, down):
    """root int64 [ny, nx]: the smallest raster index of every pixel's class under the links (an unlinked pixel: its own)."""
    ny, nx = right.shape
    n = ny * nx
    idx = np.arange(n, dtype=np.int64).reshape(ny, nx)
    a = np.concatenate([idx[right], idx[down]])
    b = np.concatenate([np.roll(idx, -1, 1)[right], np.roll(idx, -1, 0)[down]])
    parent = np.arange(n, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        apart = ra != rb
        if not apart.any():
            break
        hi, lo = np.maximum(ra[apart], rb[apart]), np.minimum(ra[apart], rb[apart])
        np.minimum.at(parent, hi, lo)
        while True:                                  # jump: every pixel to its root
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
        a, b = a[apart], b[apart]
    return parent.reshape(ny, nx)


def neighbours(state, periodic):
    """[4, ny, nx]: the state of the left, right, upper and lower neighbour position; -1 beyond a wall."""
    out = np.stack([np.roll(state, 1, 1), np.roll(state, -1, 1), np.roll(state, 1, 0), np.roll(state, -1, 0)])
    if not periodic:
        out[0, :, 0] = -1
        out[1, :, -1] = -1
        out[2, 0, :] = -1
        out[3, -1, :] = -1
    return out


def sweep(state, periodic):
    """One Jacobi sweep on state (root of a closed pixel, -1 open) -> (the next state, the pixels assigned)."""
    nb = neighbours(state, periodic)
    best, best_n = np.full(state.shape, -1, np.int64), np.zeros(state.shape, np.int64)
    for i in range(4):
        v = nb[i]
        votes = ((nb == v[None]) & (v[None] >= 0)).sum(0)
        better = (v >= 0) & ((votes > best_n) | ((votes == best_n) & (v < best)))
        best, best_n = np.where(better, v, best), np.where(better, votes, best_n)
    take = (state < 0) & (best >= 0)
    return np.where(take, best, state), int(take.sum())


def label(ids=None, angles=None, tol=None, valid=None, min_pixels=1, max_sweeps=64, boundary="periodic", grain_capacity=None):
    """-> dict: image int32 [ny, nx], n_grain, mean_angles float32 [K, min(n_grain, capacity)] or None, status (STATUS), and
    the intermediate `root` (before cleanup) and `state` (after it) for the tests that look inside."""
    assert (ids is None) != (angles is None) and boundary in ("periodic", "noflux") and min_pixels >= 1 and max_sweeps >= 0
    periodic = boundary == "periodic"
    if angles is not None:
        angles = np.asarray(angles, np.float32)
        assert angles.ndim == 3 and 1 <= angles.shape[0] <= 4 and tol is not None
        ny, nx = angles.shape[1:]
    else:
        ids = np.asarray(ids).astype(np.int32)
        ny, nx = ids.shape
    assert nx >= 3 and ny >= 3
    ok = validity(ids, angles, valid)
    right, down = links(ids, angles, tol, ok, periodic)
    root = components(right, down)
    flat = root.reshape(-1)
    size = np.bincount(flat[ok.reshape(-1)], minlength=ny * nx)
    is_root = ok & (root == np.arange(ny * nx).reshape(ny, nx))
    closed = ok & (size[flat].reshape(ny, nx) >= min_pixels)
    grain_roots = np.nonzero((is_root & closed).reshape(-1))[0]          # ascending: the numbering
    speck_roots = np.nonzero((is_root & ~closed).reshape(-1))[0]
    state = np.where(closed, root, -1).astype(np.int64)
    n_sweeps = 0
    for _ in range(max_sweeps):
        state, assigned = sweep(state, periodic)
        if not assigned:
            break
        n_sweeps += 1
    first = 1 if periodic else 2
    rank = np.full(ny * nx + 1, -first, np.int64)                       # (-1 -> 0: unfilled)
    rank[grain_roots] = np.arange(len(grain_roots))
    image = (rank[state.reshape(-1)] + first).astype(np.int32).reshape(ny, nx)
    n_grain = len(grain_roots) + (0 if periodic else 1)
    cap = ny * nx // min_pixels + 2 if grain_capacity is None else int(grain_capacity)
    means = None
    if angles is not None:
        K = angles.shape[0]
        means = np.zeros((K, min(n_grain, cap)), np.float32)
        kept = closed.reshape(-1)                                         # the ORIGINAL components: absorbed pixels do not count
        for k in range(K):
            q = np.zeros(ny * nx, np.int64)
            q[kept] = np.rint(angles[k].reshape(-1)[kept] * SCALE).astype(np.int64)
            S = np.zeros(ny * nx, np.int64)
            np.add.at(S, flat[kept], q[kept])                             # exact, whatever the order
            g = np.arange(len(grain_roots)) + (first - 1)
            m = (S[grain_roots].astype(np.float64) / size[grain_roots].astype(np.float64) / 16777216.0).astype(np.float32)
            means[k, g[g < cap]] = m[g < cap]
    status = dict(n_components=int(is_root.sum()), n_specks=len(speck_roots), n_speck_pixels=int(size[speck_roots].sum()),
                  n_invalid_in=int((~ok).sum()), n_grains=len(grain_roots), n_sweeps=n_sweeps, n_unfilled=int((state < 0).sum()),
                  overflow=int(n_grain > cap), n_bound_hits=0)
    return {"image": image, "n_grain": n_grain, "mean_angles": means, "status": status, "root": root, "state": state}


def relabel_by_first_pixel(image):
    """An id image renumbered 1, 2, .. in raster order of every id's first pixel (0 stays 0)."""
    flat = np.asarray(image).reshape(-1)
    vals, first = np.unique(flat, return_index=True)
    keep = vals > 0
    order = np.argsort(first[keep])
    lut = np.zeros(int(vals.max()) + 1, np.int32)
    lut[vals[keep][order]] = np.arange(1, keep.sum() + 1)
    return lut[np.maximum(flat, 0)].reshape(np.asarray(image).shape)


def same_partition(a, b):
    """Two label images describe the same partition of the same pixels (0 = no label in both)."""
    a, b = np.asarray(a).reshape(-1).astype(np.int64), np.asarray(b).reshape(-1).astype(np.int64)
    if not np.array_equal(a > 0, b > 0):
        return False
    pairs = np.unique(np.stack([a, b]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))


def noisy(frame, theta, d, seed):
    """The issue's noise recipe on an id frame -> (ids int32, angles float32 [K, ny, nx]): pixels with m < d / 2 non-indexed
    (id 0 / NaN), pixels with d / 2 <= m < d a wrong id from rng.integers(1, 119, count) (as that grain's angles)."""
    rng = np.random.default_rng(seed)
    m = rng.random(frame.shape)
    ids = np.asarray(frame).astype(np.int32).copy()
    ids[m < d / 2] = 0
    wrong = (m >= d / 2) & (m < d)
    ids[wrong] = rng.integers(1, 119, int(wrong.sum()))
    theta = np.asarray(theta, np.float32)
    angles = theta[:, np.maximum(ids, 1) - 1].astype(np.float32)
    angles[:, ids == 0] = np.nan
    return ids, np.ascontiguousarray(angles)
