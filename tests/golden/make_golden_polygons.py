"""Golden polygons: what the UNMODIFIED reference's traj.GNN_update -> graph.update() (graph_trajectory.py:1010-1103,
graph_datastruct.py:654-721) leaves in `regions`, `region_coors` and `region_center`, for states the other goldens of this
directory already record (so the file holds results only; the tests take the inputs from those fixtures):

  init     graph_40.npz as it is (GNN_update(0, ..., topo=True), test.py:266), on graphs/40_40/traj10020.pkl.gz as
           make_golden.py:generate_centres drives it
  step1    the junctions of golden_cfg1_centres.npz after static steps 1 and 3 (topo=False)
  step3
  mass3    the eventful update of golden_cfg1_events.npz, scenario mass3: the junctions, masks and lists Cmodel.update left
           (topo=True)
  noflux   the initial structure of noflux_40_seed1.npz on the reference's own no-flux trajectory object
           (make_golden_noflux.py: graph_trajectory(lxd=40, seed=1, BC='noflux')), boundary grain included

Runs only where the reference is (make_golden.py sets the paths up); writes polygons_cfg1.npz:
  <tag>__rowptr  int32 [n_grain + 1]   grain g (the reference's region g + 1) owns entries rowptr[g]:rowptr[g + 1]
  <tag>__regions int32 [E]             the junctions of `regions`, in its order (empty for a grain it has no region for)
  <tag>__coors   float [E, 2]          `region_coors`
  <tag>__center  float64 [n_grain, 2]  `region_center`, NaN where the reference set none (fewer than 2 junctions)
    python tests/golden/make_golden_polygons.py
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

GJ, JG, JJ = mg.GJ, mg.JG, mg.JJ
key = "__".join


def collect(out, tag, traj, n_grain):
    rowptr, regions, coors = [0], [], []
    center = np.full((n_grain, 2), np.nan)
    for g in range(n_grain):
        verts = list(traj.regions.get(g + 1, []))
        xy = [list(map(float, v)) for v in traj.region_coors.get(g + 1, [])]
        assert len(verts) == len(xy), (tag, g)
        regions += [int(v) for v in verts]
        coors += xy
        rowptr.append(len(regions))
        if g + 1 in traj.region_center:
            center[g] = [float(c) for c in traj.region_center[g + 1]]
    coors = np.asarray(coors, np.float64).reshape(-1, 2)
    if np.array_equal(coors.astype(np.float32).astype(np.float64), coors):   # (the reference moved them in float32)
        coors = coors.astype(np.float32)
    out[tag + "__rowptr"], out[tag + "__regions"] = np.asarray(rowptr, np.int32), np.asarray(regions, np.int32)
    out[tag + "__coors"], out[tag + "__center"] = coors, center
    sides = np.diff(rowptr)
    print(f"{tag}: {n_grain} grains, {int((sides > 0).sum())} with a region, sides {sides[sides > 0].min()}-{sides.max()}, "
          f"coordinates {coors.dtype}, {int(np.isfinite(center[:, 0]).sum())} centres")


def update(traj, frame, x_joint, x_grain, mask, topo, ei):
    X = {"joint": torch.from_numpy(x_joint.copy()), "grain": torch.from_numpy(x_grain.copy())}
    M = {k: torch.from_numpy(np.asarray(v).astype(np.int64).copy()) for k, v in mask.items()}
    EI = {et: torch.from_numpy(np.asarray(v).astype(np.int64).copy()) for et, v in ei.items()}
    traj.GNN_update(frame, X, M, topo, EI, False)


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
        return traj

    traj = fresh()
    update(traj, 0, g40["x_joint"], g40["x_grain"], ones, True, ei)            # test.py:266
    collect(out, "init", traj, n_g)
    for step in (1, 3):
        update(traj, step * mg.SPAN, cen[f"step{step}_x_joint"], cen[f"step{step}_x_grain"], ones, False, ei)   # test.py:478
        collect(out, f"step{step}", traj, n_g)

    traj = fresh()
    update(traj, 0, g40["x_joint"], g40["x_grain"], ones, True, ei)
    o = "mass3__out_"
    update(traj, 3 * mg.SPAN, ev[o + "x_joint"], ev[o + "x_grain"], {"grain": ev[o + "mask_grain"], "joint": ev[o + "mask_joint"]},
           True, {et: ev[o + "ei_" + key(et)] for et in mg.ETS})
    collect(out, "mass3", traj, n_g)

    nf = np.load(os.path.join(HERE, "noflux_40_seed1.npz"))
    assert float(nf["domain_factor"]) == 1.0
    traj = gt.graph_trajectory(lxd=int(nf["lxd"]), seed=1, frames=121, BC="noflux", physical_params={"G": 2.0, "R": 0.5})
    cur_grain, counts = np.unique(traj.alpha_field, return_counts=True)       # as make_golden_noflux.py:run
    traj.area_counts = dict(zip(cur_grain, counts))
    traj.area_traj.append(traj.area_counts)
    traj.form_states_tensor(0)
    traj.raise_err = False
    traj.extraV_traj = []
    update(traj, 0, nf["scaled_x_joint"], nf["scaled_x_grain"], {"grain": nf["mask_grain"], "joint": nf["mask_joint"]}, True,
           {et: nf["ei_" + key(et)] for et in mg.ETS})                          # test.py:296
    collect(out, "noflux", traj, nf["x_grain"].shape[0])

    path = os.path.join(HERE, "polygons_cfg1.npz")
    np.savez_compressed(path, **out)
    print("wrote polygons_cfg1.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
