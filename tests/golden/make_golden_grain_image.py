"""Golden grain-ID images: what the UNMODIFIED reference's traj.plot_polygons() (graph_datastruct.py:553-610, PIL's
ImageDraw.polygon) draws from `region_coors` at the trajectory's own `imagesize`, for the five states whose polygons
polygons_cfg1.npz records (make_golden_polygons.py: init, step1, step3, mass3, noflux -- the same updates in the same
order, with compare=True so that `alpha_pde` follows the frame where the trajectory carries the phase-field frames).

Runs only where the reference is (make_golden.py sets the paths up); writes grain_image_cfg1.npz:
  <tag>__alpha_field  int16 [ny, nx]   `alpha_field` after plot_polygons() (0 = uncovered)
  <tag>__alpha_pde    int16 [ny, nx]   the phase-field map compute_error_layer (:346-348) compares with
  <tag>__error_layer  float64          `error_layer`, the share of differing pixels
  <tag>__imagesize    int64 [2]        (nx, ny)
  noflux__corner_grains int64 [4]
  pil_version         the PIL that filled the polygons
    python tests/golden/make_golden_grain_image.py
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

key = "__".join


def collect(out, tag, traj, recorded):
    """plot_polygons() on the state as it is; the polygons must be the ones polygons_cfg1.npz holds for `tag`."""
    rp, coors = recorded[tag + "__rowptr"], recorded[tag + "__coors"]
    for g in range(len(rp) - 1):
        mine = np.asarray([list(map(float, v)) for v in traj.region_coors.get(g + 1, [])], np.float64).reshape(-1, 2)
        assert np.array_equal(mine, coors[rp[g]:rp[g + 1]].astype(np.float64)), (tag, g)
    traj.plot_polygons()
    field, pde = np.asarray(traj.alpha_field), np.asarray(traj.alpha_pde)
    assert field.shape == pde.shape == (traj.imagesize[1], traj.imagesize[0])
    assert 0 <= field.min() and max(field.max(), pde.max()) < 2 ** 15
    out[tag + "__alpha_field"], out[tag + "__alpha_pde"] = field.astype(np.int16), pde.astype(np.int16)
    out[tag + "__error_layer"] = np.float64(traj.error_layer)
    out[tag + "__imagesize"] = np.asarray(traj.imagesize, np.int64)
    print(f"{tag}: image {field.shape}, {int((field == 0).sum())} uncovered pixels, error_layer {traj.error_layer:.6f}")


def update(traj, frame, x_joint, x_grain, mask, topo, ei):
    X = {"joint": torch.from_numpy(x_joint.copy()), "grain": torch.from_numpy(x_grain.copy())}
    M = {k: torch.from_numpy(np.asarray(v).astype(np.int64).copy()) for k, v in mask.items()}
    EI = {et: torch.from_numpy(np.asarray(v).astype(np.int64).copy()) for et, v in ei.items()}
    traj.GNN_update(frame, X, M, topo, EI, True)


def main():
    import __main__
    import dill
    import PIL
    import graph_trajectory as gt
    __main__.graph_trajectory, __main__.graph = gt.graph_trajectory, gt.graph
    out = {"pil_version": np.asarray(PIL.__version__)}
    recorded = np.load(os.path.join(HERE, "polygons_cfg1.npz"))
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
    update(traj, 0, g40["x_joint"], g40["x_grain"], ones, True, ei)
    collect(out, "init", traj, recorded)
    for step in (1, 3):
        update(traj, step * mg.SPAN, cen[f"step{step}_x_joint"], cen[f"step{step}_x_grain"], ones, False, ei)
        collect(out, f"step{step}", traj, recorded)

    traj = fresh()
    update(traj, 0, g40["x_joint"], g40["x_grain"], ones, True, ei)
    o = "mass3__out_"
    update(traj, 3 * mg.SPAN, ev[o + "x_joint"], ev[o + "x_grain"], {"grain": ev[o + "mask_grain"], "joint": ev[o + "mask_joint"]},
           True, {et: ev[o + "ei_" + key(et)] for et in mg.ETS})
    collect(out, "mass3", traj, recorded)

    nf = np.load(os.path.join(HERE, "noflux_40_seed1.npz"))
    traj = gt.graph_trajectory(lxd=int(nf["lxd"]), seed=1, frames=121, BC="noflux", physical_params={"G": 2.0, "R": 0.5})
    cur_grain, counts = np.unique(traj.alpha_field, return_counts=True)       # as make_golden_noflux.py:run
    traj.area_counts = dict(zip(cur_grain, counts))
    traj.area_traj.append(traj.area_counts)
    traj.form_states_tensor(0)
    traj.raise_err = False
    traj.extraV_traj = []
    update(traj, 0, nf["scaled_x_joint"], nf["scaled_x_grain"], {"grain": nf["mask_grain"], "joint": nf["mask_joint"]}, True,
           {et: nf["ei_" + key(et)] for et in mg.ETS})
    out["noflux__corner_grains"] = np.asarray(traj.corner_grains, np.int64)
    collect(out, "noflux", traj, recorded)

    path = os.path.join(HERE, "grain_image_cfg1.npz")
    np.savez_compressed(path, **out)
    print("wrote grain_image_cfg1.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
