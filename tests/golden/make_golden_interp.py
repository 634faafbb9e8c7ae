"""Golden in-between layers: what the UNMODIFIED reference leaves in `regions`, `region_coors` and `region_center` when its
rollout script builds the frames of --interp_frames 2 (test.py:494-514): the junction positions of two layers blended in
torch float32 with cur_coeff = 1/3 and 2/3, move_to_boundary + the clamps (no-flux), then traj.GNN_update with the lists
and masks of the earlier layer (1/3) or the later one (2/3).  The pairs of layers are states the other goldens of this
directory already record, so the file holds results only -- except the second no-flux state, which is made here:

  static   graph_40.npz -> the junctions of golden_cfg1_centres.npz after static step 1            (same lists, topo=False)
  mass3    graph_40.npz -> the eventful update of golden_cfg1_events.npz, scenario mass3: 22 grains eliminated between
           the two layers, so 1/3 has the old lists and 2/3 the new ones                          (topo=True)
  noflux   noflux_40_seed1.npz's initial structure -> the same structure with its junctions displaced by a seeded
           N(0, 0.012) in both coordinates: wall junctions move inward and outward, junctions leave the box; stored as
           noflux__x_joint_b (an input of the tests)

Runs only where the reference is (make_golden.py sets the paths up); writes interp_cfg1.npz with, per <tag> = <pair>_<1|2>
(cur_coeff = 1/3, 2/3), the arrays make_golden_polygons.py:collect writes: <tag>__rowptr, __regions, __coors, __center.
    python tests/golden/make_golden_interp.py
"""
import gzip
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (sets up sys.path for the reference + stubs)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from make_golden_polygons import collect, key  # noqa: E402

ref_move_to_boundary = mg.ref_function("test.py", "move_to_boundary")
INTERP_FRAMES = 2
# (seed 20261 was tried first: its frame at 1/3 brings two pairs of vertices of grains 22 and 26 within 7e-4 rad of each other,
#  2 of 101 grains below the contract's gap limit, which is more than the 1 % the test may exclude; this one excludes none)
NOFLUX_SEED, NOFLUX_SIGMA = 7, 0.012


def frames(out, pair, traj, prev, cur, topo, noflux_max_y=None):
    """test.py:496-514 for one pair of layers; prev / cur = (x_joint, x_grain, mask, edge lists)."""
    tens = lambda x: torch.from_numpy(np.asarray(x).copy())
    X = {"joint": tens(cur[0]), "grain": tens(cur[1])}
    prev_X = {"joint": tens(prev[0]), "grain": tens(prev[1])}
    as_mask = lambda m: {k: tens(np.asarray(v).astype(np.int64)) for k, v in m.items()}
    as_ei = lambda ei: {et: tens(np.asarray(v).astype(np.int64)) for et, v in ei.items()}
    for interp_frame in range(INTERP_FRAMES):
        cur_coeff = (1 + interp_frame) / (1 + INTERP_FRAMES)
        pre_coeff = 1 - cur_coeff
        mean_X = {k: v.clone() for k, v in X.items()}
        mean_X["joint"][:, :2] = cur_coeff * X["joint"][:, :2] + pre_coeff * prev_X["joint"][:, :2]
        side = cur if cur_coeff > 0.5 else prev
        ei = as_ei(side[3])
        if noflux_max_y is not None:   # (departure 1 of DESIGN.md 8i: the script calls it on periodic graphs too)
            ref_move_to_boundary(mean_X["joint"], ei[mg.GJ], [1, noflux_max_y])
            mean_X["joint"][:, 0] = torch.clamp(mean_X["joint"][:, 0], min=0, max=1)
            mean_X["joint"][:, 1] = torch.clamp(mean_X["joint"][:, 1], min=0, max=noflux_max_y)
        traj.GNN_update(6, mean_X, as_mask(side[2]), topo, ei, False)
        collect(out, f"{pair}_{interp_frame + 1}", traj, np.asarray(cur[1]).shape[0])


def main():
    import __main__
    import dill
    import graph_trajectory as gt
    __main__.graph_trajectory, __main__.graph = gt.graph_trajectory, gt.graph
    out = {}
    g40 = np.load(os.path.join(HERE, "graph_40.npz"))
    cen = np.load(os.path.join(HERE, "golden_cfg1_centres.npz"))
    ev = np.load(os.path.join(HERE, "golden_cfg1_events.npz"))
    ei = {et: g40["ei_" + key(et)] for et in mg.ETS}
    n_g, n_j = g40["x_grain"].shape[0], g40["x_joint"].shape[0]
    ones = {"grain": np.ones((n_g, 1), np.int64), "joint": np.ones((n_j, 1), np.int64)}

    def fresh():
        with gzip.open(os.path.join(mg.REF, "graphs/40_40/traj10020.pkl.gz"), "rb") as f:
            traj = dill.load(f)
        traj.raise_err = False
        traj.extraV_traj, traj.area_traj = [], traj.area_traj[:1]
        X = {"joint": torch.from_numpy(g40["x_joint"].copy()), "grain": torch.from_numpy(g40["x_grain"].copy())}
        traj.GNN_update(0, X, {k: torch.from_numpy(v) for k, v in ones.items()}, True,
                        {et: torch.from_numpy(v.astype(np.int64)) for et, v in ei.items()}, False)   # test.py:266
        return traj

    init = (g40["x_joint"], g40["x_grain"], ones, ei)
    frames(out, "static", fresh(), init, (cen["step1_x_joint"], cen["step1_x_grain"], ones, ei), False)
    o = "mass3__out_"
    frames(out, "mass3", fresh(), init,
           (ev[o + "x_joint"], ev[o + "x_grain"], {"grain": ev[o + "mask_grain"], "joint": ev[o + "mask_joint"]},
            {et: ev[o + "ei_" + key(et)] for et in mg.ETS}), True)

    nf = np.load(os.path.join(HERE, "noflux_40_seed1.npz"))
    assert float(nf["domain_factor"]) == 1.0
    traj = gt.graph_trajectory(lxd=int(nf["lxd"]), seed=1, frames=121, BC="noflux", physical_params={"G": 2.0, "R": 0.5})
    cur_grain, counts = np.unique(traj.alpha_field, return_counts=True)       # as make_golden_noflux.py:run
    traj.area_counts = dict(zip(cur_grain, counts))
    traj.area_traj.append(traj.area_counts)
    traj.form_states_tensor(0)
    traj.raise_err = False
    traj.extraV_traj = []
    nf_mask = {"grain": nf["mask_grain"], "joint": nf["mask_joint"]}
    nf_ei = {et: nf["ei_" + key(et)] for et in mg.ETS}
    moved = nf["scaled_x_joint"].copy()
    moved[:, :2] += np.random.RandomState(NOFLUX_SEED).normal(0.0, NOFLUX_SIGMA, (moved.shape[0], 2)).astype(np.float32)
    out["noflux__x_joint_b"] = moved[:, :2].copy()
    first = (nf["scaled_x_joint"], nf["scaled_x_grain"], nf_mask, nf_ei)
    X0 = {"joint": torch.from_numpy(first[0].copy()), "grain": torch.from_numpy(first[1].copy())}
    traj.GNN_update(0, X0, {k: torch.from_numpy(np.asarray(v).astype(np.int64)) for k, v in nf_mask.items()}, True,
                    {et: torch.from_numpy(v.astype(np.int64)) for et, v in nf_ei.items()}, False)       # test.py:296
    frames(out, "noflux", traj, first, (moved, nf["scaled_x_grain"], nf_mask, nf_ei), True, noflux_max_y=float(nf["max_y"]))

    path = os.path.join(HERE, "interp_cfg1.npz")
    np.savez_compressed(path, **out)
    print("wrote interp_cfg1.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
