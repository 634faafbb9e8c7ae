"""Golden (G, R) schedules of the reference's `--temporal` mode: graph_trajectory.GR_seq_from_time (graph_trajectory.py:129-155,
with TemperatureProfile3DAnalytic.RandGR, :18-43) of the UNMODIFIED reference, imported at run time through tools/oracle_stub,
for three (seed, freq) pairs -- test.py:346 calls it with freq = 2 ** (seed % 10), delta_z = train_delta_z * span and the
trajectory's heights (2 and 50 um by default).

Runs only in the build container (needs /root/reference); writes data only:
    python tests/golden/make_golden_gr_schedule.py
      gr_schedule.npz   seeds, freqs [3] int64; ini_height, final_height, delta_z float64; G_<i>, R_<i> [counts] float64

The method draws from numpy's global stream, reads four attributes of its object and saves a figure into the working
directory: it is called on a bare object with those attributes, inside a temporary directory.
"""
import os
import sys
import tempfile

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402,F401  (sets up sys.path for the reference + stubs)
import numpy as np  # noqa: E402

SPAN = 6
TRAIN_DELTA_Z = 0.4   # test.py:191
INI_HEIGHT, FINAL_HEIGHT = 2, 50
PAIRS = [(10020, 2 ** (10020 % 10)), (3, 2 ** (3 % 10)), (5, 3)]   # test.py:346's rule twice, one free pair


def schedule(gt, seed, freq):
    traj = object.__new__(gt.graph_trajectory)
    traj.seed, traj.ini_height, traj.final_height, traj.physical_params = seed, INI_HEIGHT, FINAL_HEIGHT, {}
    frames = int((traj.final_height - traj.ini_height) / TRAIN_DELTA_Z) + 1          # test.py:307
    traj.GR_seq_from_time(seed, freq, TRAIN_DELTA_Z * SPAN, (frames - 1) // SPAN)    # test.py:346
    return np.asarray(traj.G_list, np.float64), np.asarray(traj.R_list, np.float64)


if __name__ == "__main__":
    import graph_trajectory as gt
    out = {"seeds": np.asarray([s for s, _ in PAIRS], np.int64), "freqs": np.asarray([f for _, f in PAIRS], np.int64),
           "ini_height": np.float64(INI_HEIGHT), "final_height": np.float64(FINAL_HEIGHT),
           "delta_z": np.float64(TRAIN_DELTA_Z * SPAN)}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for i, (seed, freq) in enumerate(PAIRS):
                out[f"G_{i}"], out[f"R_{i}"] = schedule(gt, seed, freq)
        finally:
            os.chdir(cwd)
    path = os.path.join(HERE, "gr_schedule.npz")
    np.savez_compressed(path, **out)
    print(f"wrote gr_schedule.npz: {os.path.getsize(path)} bytes, rows {[len(out[f'G_{i}']) for i in range(len(PAIRS))]}")
