"""The linking rule of include/ggnn.h (ggnn_link_labels), restated by brute force in numpy: a stack of labelled frames, each in
its own numbering, -> the stack in ids that persist from frame to frame, the per-frame gid and pred rows, first_frame,
last_frame, theta and the status words.  No kernel, no slots: the votes are one np.bincount over the (b, a) pairs of a pair of
frames, the matcher is a loop over the grains, the global ids are composed frame after frame."""
import numpy as np

FRAME_WORDS = ("n_local", "n_matched", "n_fresh", "n_split", "n_gone", "n_vote_overflow")
GLOBAL_WORDS = ("n_global", "overflow")


def first_id(boundary):
    assert boundary in ("periodic", "noflux")
    return 1 if boundary == "periodic" else 2


def votes(before, cur, first, La, Lb):
    """int64 [Lb, La]: vote[b - first, a - first] = the pixels that hold local grain b now and local grain a before."""
    a, b = before.reshape(-1).astype(np.int64) - first, cur.reshape(-1).astype(np.int64) - first
    both = (a >= 0) & (a < La) & (b >= 0) & (b < Lb)
    return np.bincount(b[both] * La + a[both], minlength=La * Lb).reshape(Lb, La)


def match(vote, min_overlap=1, mean_b=None, mean_a=None, match_tol=None):
    """The predecessor rows of one pair of frames from its votes -> (pred rows [Lb] (row a - first, or -1), n_split, n_gone)."""
    Lb, La = vote.shape
    pred = np.full(Lb, -1, np.int64)
    for b in range(Lb):
        ok = vote[b] >= min_overlap
        if match_tol is not None:
            with np.errstate(invalid="ignore"):
                d = np.abs(mean_b[:, b, None].astype(np.float32) - mean_a.astype(np.float32))   # one fp32 subtraction a channel
                ok &= np.all(d <= np.float32(match_tol), axis=0)
        if ok.any():
            pred[b] = int(np.argmax(np.where(ok, vote[b], -1)))      # (argmax: the first of equal ones, the smaller a)
    n_split = 0
    for a in range(La):
        claimants = np.nonzero(pred == a)[0]
        if len(claimants) > 1:
            keeper = claimants[int(np.argmax(vote[claimants, a]))]   # (the first of equal ones: the smaller b)
            for b in claimants:
                if b != keeper:
                    pred[b] = -1
                    n_split += 1
    n_gone = La - len(np.unique(pred[pred >= 0]))
    return pred, n_split, n_gone


def link(labels, n_local, means=None, match_tol=None, min_overlap=1, boundary="periodic", local_capacity=None, global_capacity=None):
    """-> dict: frames int32 [T, ny, nx], gid and pred int32 [T, local_capacity], first_frame and last_frame int32
    [global_capacity], theta float32 [K, global_capacity] or None, status (per frame dicts of FRAME_WORDS), n_global, overflow,
    n_grain, and `candidates` (per pair, the largest number of grains of the frame before that one grain overlaps)."""
    labels = np.asarray(labels).astype(np.int32)
    T, ny, nx = labels.shape
    first = first_id(boundary)
    n_local = [int(n) for n in np.asarray(n_local).reshape(-1)]
    assert T >= 1 and len(n_local) == T and min_overlap >= 1
    Lc = max(max(n_local), 1) if local_capacity is None else int(local_capacity)
    Gc = Lc * min(T, 2) if global_capacity is None else int(global_capacity)
    K = 0 if means is None else np.asarray(means).shape[1]
    if K:
        means = np.asarray(means, np.float32)
        assert means.shape == (T, K, Lc)
    assert match_tol is None or (K > 0 and match_tol >= 0)
    L = [min(max(n, 0), Lc) for n in n_local]
    overflow = sum(1 for n in n_local if n < 0 or n > Lc)
    gid, pred = np.zeros((T, Lc), np.int32), np.full((T, Lc), -1, np.int32)
    first_frame, last_frame = np.full(Gc, -1, np.int32), np.full(Gc, -1, np.int32)
    theta = np.zeros((K, Gc), np.float32) if K else None
    status = [dict.fromkeys(FRAME_WORDS, 0) for _ in range(T)]
    candidates = []

    def born(t, i, g):
        if g < Gc:
            first_frame[g] = last_frame[g] = t
            if K:
                theta[:, g] = means[t, :, i]

    n_global = L[0]
    status[0]["n_local"] = L[0]
    for i in range(L[0]):
        gid[0, i] = first + i
        born(0, i, i)
    for t in range(1, T):
        v = votes(labels[t - 1], labels[t], first, L[t - 1], L[t])
        candidates.append(int((v > 0).sum(1).max()) if v.size else 0)
        p, n_split, n_gone = match(v, min_overlap, means[t][:, :L[t]] if K else None, means[t - 1][:, :L[t - 1]] if K else None, match_tol)
        fresh = 0
        for i in range(L[t]):
            if p[i] >= 0:
                pred[t, i] = p[i] + first
                g = int(gid[t - 1, p[i]]) - first
                if g < Gc:
                    last_frame[g] = t
            else:
                g = n_global + fresh
                fresh += 1
                born(t, i, g)
            gid[t, i] = g + first
        n_global += fresh
        status[t].update(n_local=L[t], n_matched=L[t] - fresh, n_fresh=fresh, n_split=n_split, n_gone=n_gone)
    frames = np.zeros_like(labels)
    for t in range(T):
        row = labels[t].astype(np.int64) - first
        local = (row >= 0) & (row < L[t])
        lut = np.concatenate([gid[t, :L[t]], [0]]).astype(np.int32)
        frames[t] = lut[np.where(local, row, L[t])]
        if first == 2:
            frames[t][labels[t] == 1] = 1
        overflow += int((~local & (labels[t] != 0) & ~((labels[t] == 1) & (first == 2))).sum())
    overflow += int(n_global > Gc)
    return {"frames": frames, "gid": gid, "pred": pred, "first_frame": first_frame, "last_frame": last_frame, "theta": theta,
            "status": status, "n_global": n_global, "overflow": overflow, "n_grain": n_global + (first - 1), "candidates": candidates}


def status_words(r):
    """The status as the call writes it: FRAME_WORDS per frame, then GLOBAL_WORDS."""
    return [s[k] for s in r["status"] for k in FRAME_WORDS] + [r["n_global"], r["overflow"]]


def renumber(labels, seed, boundary="periodic"):
    """Every frame of a stack of labelled frames in a random numbering of its own -> (the stack, n_local per frame); ids below
    `first` stay."""
    first, rs = first_id(boundary), np.random.RandomState(seed)
    out, n_local = np.array(labels, np.int32), []
    for t, frame in enumerate(out):
        ids = np.unique(frame[frame >= first])
        lut = np.arange(int(frame.max()) + 1, dtype=np.int32)
        lut[ids] = first + rs.permutation(len(ids))
        out[t] = lut[np.maximum(frame, 0)]
        n_local.append(len(ids))
    return out, n_local
