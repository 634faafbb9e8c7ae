"""numpy restatement of ggnn_process_schedule (include/ggnn.h) and the problems its tests run on.

restate(x, table, off, counter) is the launch on host arrays: every junction j of trajectory t gets
x[j, 3] = table[r, t, 0], x[j, 4] = table[r, t, 1] with r = min(max(counter + 1, 0), n_rows - 1), t = the LAST trajectory
whose offset is <= j (empty trajectories are stepped over), and the counter becomes counter + 1.  It copies fp32 values:
the kernel is compared with np.array_equal.

`variant` names a deliberate mistake (test_process_schedule.py proves that the bit-for-bit comparison on these problems
rejects each of them):
  row_k       the row of the counter itself instead of the step to come
  no_clamp    no clamp at the table's end: whatever lies behind the last row
  prev_traj   a trajectory's first junction takes the trajectory of the junction before it
  col2, col5  one more column written
"""
import numpy as np

VARIANTS = ("row_k", "no_clamp", "prev_traj", "col2", "col5")
F_JOINT = 8           # junction features of the models
GUARD = 3             # sentinel rows in front of and behind x
BEHIND_TABLE = -7.25  # what the no_clamp mistake reads behind the last row


def trajectory_of(off, n_joint, variant=None):
    """[n_joint] the trajectory of every junction: the last offset <= j."""
    j = np.arange(n_joint)
    if off is None:
        return np.zeros(n_joint, np.int64)
    off = np.asarray(off, np.int64)
    t = np.searchsorted(off[:-1], j, side="right") - 1
    if variant == "prev_traj":
        first = np.isin(j, off[:-1]) & (j > 0)
        t = np.where(first, np.searchsorted(off[:-1], np.maximum(j - 1, 0), side="right") - 1, t)
    return t


def restate(x, table, off, counter, variant=None):
    """-> (x after the launch, counter after the launch).  x: [n_joint, ldx] fp32 (not modified); table: [n_rows, n_traj, 2]
    fp32; off: [n_traj + 1] or None (one trajectory)."""
    assert variant is None or variant in VARIANTS, variant
    x, table = np.array(x, np.float32, copy=True), np.asarray(table, np.float32)
    n_rows = table.shape[0]
    r = counter if variant == "row_k" else counter + 1
    r = max(r, 0)
    if variant == "no_clamp":
        table = np.concatenate([table, np.full((max(r + 1 - n_rows, 0),) + table.shape[1:], BEHIND_TABLE, np.float32)])
    else:
        r = min(r, n_rows - 1)
    t = trajectory_of(off, x.shape[0], variant)
    x[:, 3], x[:, 4] = table[r, t, 0], table[r, t, 1]
    if variant == "col2":
        x[:, 2] = table[r, t, 0]
    if variant == "col5":
        x[:, 5] = table[r, t, 1]
    return x, counter + 1


def problem(sizes, n_rows, pad=0, seed=7):
    """A launch's operands: x [GUARD + n_joint + GUARD, F_JOINT + pad] of distinct sentinel values (the launch sees the
    middle rows), a table [n_rows, n_traj, 2] of distinct values and the offsets (None for sizes=None-like single ints)."""
    rs = np.random.RandomState(seed)
    single = np.isscalar(sizes)
    sizes = [int(sizes)] if single else [int(s) for s in sizes]
    n = sum(sizes)
    ldx = F_JOINT + pad
    whole = (1000.0 + np.arange((n + 2 * GUARD) * ldx, dtype=np.float64)).astype(np.float32).reshape(-1, ldx)
    table = rs.uniform(-1.0, 1.0, (n_rows, len(sizes), 2)).astype(np.float32)
    assert len(np.unique(table)) == table.size
    off = None if single else np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return whole, table, off


UNION_SIZES = (1, 63, 64, 65, 0, 255, 257)   # boundaries inside a wave, on a wave edge, inside and across blocks; one empty


def many_small(n_traj=600, seed=3):
    """More trajectories than the kernel stages in LDS: 1-3 junctions each."""
    return np.random.RandomState(seed).randint(1, 4, n_traj).tolist()
