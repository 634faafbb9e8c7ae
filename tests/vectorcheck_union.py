"""The union of a stack of grain-ID images (ggnn_image_junctions_traj / ggnn_junction_links_traj, include/ggnn.h), restated:
tests/vectorcheck.py (periodic) or tests/vectorcheck_noflux.py (no-flux) per image, concatenated with the offsets.

  grains     image b's local grain g is union grain grain_off[b] + g
  junctions  image after image; image b's begin at joint_off[b] = the junctions of the images before it
  capacity   the union's: junction j is kept when j < joint_capacity, so image b keeps its first joint_capacity - joint_off[b];
             its status is that of its own call with that much room (n_open_pairs counts the pairs whose partner was cut off),
             an image that begins at or beyond the capacity keeps nothing and links nothing, and overflow is 1 for every image
             whose last junction lies beyond the capacity
  counts     np.bincount of every image, ids 1 .. n_grain"""
import numpy as np

import vectorcheck as vc
import vectorcheck_noflux as vn

STATUS = vc.STATUS


def vectorize(images, n_grains, grid="cells", merge_radius=2, joint_capacity=None, boundary="periodic"):
    """-> dict of the union's xy float32 [n, 2], triples int32 [n, 3], gj / jj int64 [2, 3 n] (n = min(n_joint, capacity)),
    status (a list of dicts), grain_off, joint_off (not clamped), counts int64 [sum(n_grains)], and for no-flux corner_grains
    (a list of 4-tuples) and max_y."""
    one = vc.vectorize if boundary == "periodic" else vn.vectorize
    n_grains = [int(n) for n in n_grains]
    assert len(images) == len(n_grains) and len({np.asarray(i).shape for i in images}) == 1
    grain_off = [0]
    for n in n_grains:
        grain_off.append(grain_off[-1] + n)
    cap = 3 * grain_off[-1] + 16 * len(images) if joint_capacity is None else int(joint_capacity)
    full = [one(image, n, grid, merge_radius=merge_radius, joint_capacity=1 << 30) for image, n in zip(images, n_grains)]
    joint_off = [0]
    for v in full:
        joint_off.append(joint_off[-1] + v["status"]["n_joint"])
    xy, triples, gj, jj, status, counts = [], [], [], [], [], []
    for b, (image, n, v) in enumerate(zip(images, n_grains, full)):
        room = cap - joint_off[b]
        if room >= 1:
            if v["status"]["n_joint"] > room:
                v = one(image, n, grid, merge_radius=merge_radius, joint_capacity=room)
            s = dict(v["status"])
            shift_g, shift_j = grain_off[b], joint_off[b]
            xy.append(v["xy"])
            triples.append(v["triples"] + np.int32(shift_g))
            gj.append(v["gj"] + np.array([[shift_g], [shift_j]], np.int64))
            own = v["jj"].copy()
            own[0] += shift_j
            own[1] = np.where(own[1] >= 0, own[1] + shift_j, own[1])
            jj.append(own)
        else:
            s = dict(v["status"], n_open_pairs=0)
        s["overflow"] = int(joint_off[b + 1] > cap)
        status.append(s)
        img = np.asarray(image).astype(np.int64).ravel()
        counts.append(np.bincount(img[(img >= 1) & (img <= n)], minlength=n + 1)[1:].astype(np.int64))
    out = {"xy": np.concatenate(xy).astype(np.float32).reshape(-1, 2), "triples": np.concatenate(triples).astype(np.int32).reshape(-1, 3),
           "gj": np.concatenate(gj, 1).astype(np.int64), "jj": np.concatenate(jj, 1).astype(np.int64), "status": status,
           "grain_off": grain_off, "joint_off": joint_off, "counts": np.concatenate(counts)}
    if boundary == "noflux":
        out["corner_grains"] = [v["corner_grains"] for v in full]
        out["max_y"] = full[0]["max_y"]
    return out
