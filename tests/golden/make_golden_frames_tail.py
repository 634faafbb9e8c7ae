"""Two more frames of the recorded sequence of pf_frames_cfg1.npz (make_golden_frames.py), for linking by tracing boundaries
(vectorize.frames_to_samples(links="trace"), tests/test_trace_links.py): frames 42 and 48 of the trajectory
graphs/40_40/traj10020.pkl.gz.  With pf_frames_cfg1.npz they make the sequence 0, 6, .., 48: frame 36, the fixture's last one, holds
a grain that is a lens on a boundary one frame before the reference eliminates it, and the frames behind it are what the pairs
(36, 42) and (42, 48) need.

Runs only where the reference is (make_golden.py sets the paths up and provides the import stubs); only run-time DATA of the
reference is written, to pf_frames_cfg1_tail.npz:
  frames        int8 [2, 501, 501]   alpha_pde_frames[:, :, f].T for f = 42, 48, pixel p = grain p - 1, ids 1 .. 118
  frame_ids     int64 [2]
  extra_volume  float64 [2, 118]     extraV_frames[:, f] / 501**3
  event_frame, event_grain int64 [n] grain_events of frames 37 .. 48, flat: grain event_grain[i] (the reference's 1-based id) is
                                     eliminated at frame event_frame[i]
    python tests/golden/make_golden_frames_tail.py
"""
import gzip
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (sets up sys.path for the reference + stubs)
import numpy as np  # noqa: E402

FRAMES = [42, 48]
AFTER = 36                      # the last frame of pf_frames_cfg1.npz


def main():
    import __main__
    import dill
    import graph_trajectory as gt
    __main__.graph_trajectory, __main__.graph = gt.graph_trajectory, gt.graph
    with gzip.open(os.path.join(mg.REF, "graphs/40_40/traj10020.pkl.gz"), "rb") as f:
        traj = dill.load(f)
    alpha = np.asarray(traj.alpha_pde_frames)
    assert alpha.shape == (501, 501, 121) and alpha.min() >= 1 and alpha.max() <= 118
    head = np.load(os.path.join(HERE, "pf_frames_cfg1.npz"))
    assert int(head["frame_ids"][-1]) == AFTER and np.array_equal(head["frames"][-1], alpha[:, :, AFTER].T), "the same trajectory"
    frames = np.stack([alpha[:, :, f].T for f in FRAMES]).astype(np.int8)
    extra = np.asarray(traj.extraV_frames, np.float64)[:, FRAMES].T / 501.0 ** 3
    ef, eg = [], []
    for f in range(AFTER + 1, FRAMES[-1] + 1):
        for g in sorted(int(g) for g in traj.grain_events[f]):
            ef.append(f)
            eg.append(g)
    out = {"frames": frames, "frame_ids": np.asarray(FRAMES, np.int64), "extra_volume": np.ascontiguousarray(extra),
           "event_frame": np.asarray(ef, np.int64), "event_grain": np.asarray(eg, np.int64)}
    path = os.path.join(HERE, "pf_frames_cfg1_tail.npz")
    np.savez_compressed(path, **out)
    print("wrote pf_frames_cfg1_tail.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
