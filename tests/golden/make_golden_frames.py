"""A recorded sequence of grain-ID images for the frame tracker (vectorize.frames_to_samples, tests/test_track.py): every sixth
phase-field frame -- the reference's span for this (G, R) -- of the trajectory graphs/40_40/traj10020.pkl.gz, frames 0 .. 36.

Runs only where the reference is (make_golden.py sets the paths up and provides the import stubs); only run-time DATA of the
reference is written, to pf_frames_cfg1.npz:
  frames        int8 [7, 501, 501]   alpha_pde_frames[:, :, f].T for f = 0, 6, .., 36 (the orientation of grain_image_cfg1.npz's
                                     init__alpha_pde), pixel p = grain p - 1, ids 1 .. 118
  frame_ids     int64 [7]
  extra_volume  float64 [7, 118]     extraV_frames[:, f] / 501**3
  theta_x, theta_z float64 [118]     the trajectory's angles without the boundary grain's entry 0
  G, R          float64
  event_frame, event_grain int64 [n] grain_events of frames 1 .. 36, flat: grain event_grain[i] (the reference's 1-based id) is
                                     eliminated at frame event_frame[i]
and, per emitted pair t = 0 .. 4, what the reference's OWN GrainHeterograph.form_gradient (graph_datastruct.py:851-1011) makes of
the two states (prev=None, nxt=the next state):
  fg<t>__y_grain      float64 [118, 2]  target_dicts['grain']
  fg<t>__y_joint      float64 [n_t, 2]  mask['joint'] * target_dicts['joint'] (an unmatched row of the reference holds the
                                        difference to a row that does not exist; the mask is how its loss reads the target)
  fg<t>__mask_joint   int64 [n_t]       mask['joint'] after the call
  fg<t>__grain_event  int64 [118]       target_dicts['grain_event']
  fg<t>__wrapped      int64 [k]         the matched junctions whose raw difference exceeds 0.5 in a coordinate
The two states are built from the restatement's output (tests/vectorcheck_union.py, tests/trackcheck.py): features in float64 --
positions the float64 of the junctions' fp32 coordinates, areas count / 501**2, extraV the fixture's --, `vertex2joint` the
triples, frame t + 1's junctions numbered BY THEIR MATCH (row i of the next state is the partner of junction i; an unmatched
junction of frame t+1 gets a fresh index behind those of frame t).  form_gradient asserts |mask * target| < 1 (:961), which
the raw difference of a junction that crossed a periodic wall breaks (+-5): the maker FEEDS IT THE WRAPPED NEXT POSITION for
those rows (position + minimum-image difference) and lists them in fg<t>__wrapped; the asserts themselves are left in force.
form_gradient also needs a junction-junction edge to take maxima over: both states carry one dummy edge, which no stored
array depends on.
    python tests/golden/make_golden_frames.py
"""
import gzip
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (sets up sys.path for the reference + stubs)
import numpy as np  # noqa: E402

FRAMES = list(range(0, 37, 6))


def state(gd, xy, area, extra_v, mask_grain, vertex2joint, n_rows):
    """A GrainHeterograph with what form_gradient reads."""
    g = gd.GrainHeterograph()
    fg = np.zeros((len(area), 10))
    fg[:, 3], fg[:, 4] = area, extra_v
    fj = np.zeros((n_rows, 6))
    fj[:len(xy), :2] = xy
    g.feature_dicts = {"grain": fg, "joint": fj}
    g.mask = {"grain": mask_grain.astype(int).reshape(-1, 1), "joint": np.zeros((n_rows, 1), int)}
    for i in vertex2joint:
        g.mask["joint"][i, 0] = 1
    g.vertex2joint = dict(vertex2joint)
    g.edges = [[0, 1]]
    g.edge_weight_dicts = {g.edge_type[2]: np.full((1, 1), 0.1)}
    g.span = 6
    return g


def form_gradient_goldens(frames, extra, G, R):
    sys.path.insert(0, os.path.dirname(HERE))
    import graph_datastruct as gd
    import trackcheck as tc
    import vectorcheck_union as vu
    T, n_grain, pp = len(frames), 118, 501.0 * 501.0
    u = vu.vectorize(list(frames), [n_grain] * T, grid="points")
    r = tc.track(u, n_grain, "periodic", patch_pixels=pp, extra_volume=extra)
    counts = u["counts"].astype(np.float64).reshape(T, n_grain)
    xy = u["xy"].astype(np.float64)
    out = {}
    for t, _ in r["pairs"]:
        j0, j1, j2 = r["joint_off"][t], r["joint_off"][t + 1], r["joint_off"][t + 2]
        n_t = j1 - j0
        local = lambda j, f: tuple(int(g) - f * n_grain for g in u["triples"][j])
        cur = state(gd, xy[j0:j1], counts[t] / pp, extra[t], counts[t] != 0, {j - j0: local(j, t) for j in range(j0, j1)}, n_t)
        fresh = [k for k in range(j1, j2) if r["prev"][k] < 0]
        row = {int(r["next"][j]): j - j0 for j in range(j0, j1) if r["next"][j] >= 0}
        row.update({k: n_t + i for i, k in enumerate(fresh)})
        nxy, wrapped = np.zeros((n_t + len(fresh), 2)), []
        for k, i in row.items():
            nxy[i] = xy[k]
            if i < n_t:
                d = xy[k] - xy[j0 + i]
                if (np.abs(d) > 0.5).any():
                    wrapped.append(i)
                    nxy[i] = xy[j0 + i] + np.where(d > 0.5, d - 1.0, np.where(d < -0.5, d + 1.0, d))
        nxt = state(gd, nxy, counts[t + 1] / pp, extra[t + 1], counts[t + 1] != 0, {i: local(k, t + 1) for k, i in row.items()},
                    len(nxy))
        cur.form_gradient(None, nxt, [], [])
        key = f"fg{t}__"
        out[key + "y_grain"] = np.asarray(cur.target_dicts["grain"], np.float64)
        out[key + "y_joint"] = np.asarray(cur.mask["joint"] * cur.target_dicts["joint"], np.float64)
        out[key + "mask_joint"] = np.asarray(cur.mask["joint"][:, 0], np.int64)
        out[key + "grain_event"] = np.asarray(cur.target_dicts["grain_event"], np.int64)
        out[key + "wrapped"] = np.asarray(wrapped, np.int64)
        print(f"pair {t}: {int(out[key + 'mask_joint'].sum())} of {n_t} junctions kept, {len(wrapped)} wrapped, "
              f"{int(out[key + 'grain_event'].sum())} grain events")
    return out


def main():
    import __main__
    import dill
    import graph_trajectory as gt
    __main__.graph_trajectory, __main__.graph = gt.graph_trajectory, gt.graph
    with gzip.open(os.path.join(mg.REF, "graphs/40_40/traj10020.pkl.gz"), "rb") as f:
        traj = dill.load(f)
    alpha = np.asarray(traj.alpha_pde_frames)
    assert alpha.shape == (501, 501, 121) and alpha.min() >= 1 and alpha.max() <= 118
    frames = np.stack([alpha[:, :, f].T for f in FRAMES]).astype(np.int8)
    first = np.load(os.path.join(HERE, "grain_image_cfg1.npz"))["init__alpha_pde"]
    assert np.array_equal(frames[0], first), "frame 0 is the image grain_image_cfg1.npz holds"
    extra = np.asarray(traj.extraV_frames, np.float64)[:, FRAMES].T / 501.0 ** 3
    ef, eg = [], []
    for f in range(1, FRAMES[-1] + 1):
        for g in sorted(int(g) for g in traj.grain_events[f]):
            ef.append(f)
            eg.append(g)
    out = {"frames": frames, "frame_ids": np.asarray(FRAMES, np.int64), "extra_volume": np.ascontiguousarray(extra),
           "theta_x": np.asarray(traj.theta_x, np.float64)[1:], "theta_z": np.asarray(traj.theta_z, np.float64)[1:],
           "G": np.float64(traj.physical_params["G"]), "R": np.float64(traj.physical_params["R"]),
           "event_frame": np.asarray(ef, np.int64), "event_grain": np.asarray(eg, np.int64)}
    out.update(form_gradient_goldens(frames.astype(np.int32), extra, float(out["G"]), float(out["R"])))
    path = os.path.join(HERE, "pf_frames_cfg1.npz")
    np.savez_compressed(path, **out)
    print("wrote pf_frames_cfg1.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
