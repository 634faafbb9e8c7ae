"""Golden quantities of interest (grain volumes, size statistics) of three rollouts of the UNMODIFIED reference, imported at
run time through tools/oracle_stub: GNN_update's "qoi" bookkeeping (graph_trajectory.py:1042-1051) at every frame, then
volume('graph') (:221-242) and the arithmetic of qoi() up to the histogram (:244-256), without plotting.

Runs only in the build container (needs /root/reference); writes data only:
    python tests/golden/make_golden_qoi.py
      qoi_cfg1_events.npz   the 40 um event trajectory of make_golden_events.py (seeded weights, real Cmodel.update), 5 steps
      qoi_noflux_40_seed1.npz   make_golden_noflux.py's 40 um no-flux trajectory, its own loop, 6 steps
      qoi_cfg1_static.npz   the 40 um graph, static topology (make_golden.py's loop (4)), 20 steps

Per file, L = number of steps, N = number of grains:
  xg34 [L+1, N, 2] fp32     x_grain[:, 3:5] as GNN_update saw them (layer 0 = the initial state)
  mask [L+1, N] int64        the grain mask it saw
  area0 [N] fp64             area_traj[0]: the rasterised pixel counts the reference keeps there (test.py:340)
  area_traj [L+1, N], extraV_traj [L+1, N], volume_traj [L+1, N] fp64 (a grain without an entry in a layer's dict: 0)
  grain_size [N], d_mu, d_std, hist_density, hist_counts, bin_edges
  patch_size, mesh_size, ini_height, final_height, frames, span, lxd, num_regions
"""
import gzip
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (sets up sys.path for the reference + stubs)
import make_golden_events as mge  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

GJ, JG, JJ = mg.GJ, mg.JG, mg.JJ
SPAN = 6
TRAIN_DELTA_Z = 0.4   # test.py:191


class Recorder:
    """What GNN_update is handed at every frame: wraps the bound method of one trajectory object."""

    def __init__(self, traj):
        self.traj, self.xg, self.mask = traj, [], []
        self.inner = traj.GNN_update
        traj.GNN_update = self

    def __call__(self, frame, x_dict, mask, topo, edge_index_dict, compare):
        self.xg.append(x_dict["grain"][:, 3:5].detach().numpy().astype(np.float32).copy())
        self.mask.append(np.asarray(mask["grain"][:, 0].detach().numpy(), np.int64).copy())
        return self.inner(frame, x_dict, mask, topo, edge_index_dict, compare)


def dense(counts, n):
    out = np.zeros(n, np.float64)
    for grain, area in counts.items():
        assert 1 <= grain <= n, grain   # (volume() indexes grain - 1)
        out[grain - 1] = area
    return out


def finish(traj, rec, out_name):
    """test.py:278-307, 340 (settings), :589-600 (traj.qoi(mode='graph')) without the figure."""
    n = rec.xg[0].shape[0]
    traj.span = SPAN
    traj.imagesize = (int(traj.lxd / traj.mesh_size) + 1, int(traj.lxd / traj.mesh_size) + 1)
    traj.frames = int((traj.final_height - traj.ini_height) / TRAIN_DELTA_Z) + 1
    assert len(traj.area_traj) == len(traj.extraV_traj) == len(rec.xg)
    traj.volume("graph")
    grain_size = np.cbrt(6 * traj.volume_traj[-1] / np.pi) * traj.mesh_size
    d_mu, d_std = np.mean(grain_size), np.std(grain_size)
    step = 1 if traj.num_regions > 400 else 2
    bins = np.arange(0, 20, step)
    dis, bin_edge = np.histogram(grain_size, bins, density=True)
    counts, _ = np.histogram(grain_size, bins)
    out = {
        "xg34": np.stack(rec.xg), "mask": np.stack(rec.mask), "area0": dense(traj.area_traj[0], n),
        "area_traj": np.stack([dense(c, n) for c in traj.area_traj]),
        "extraV_traj": np.stack([np.asarray(e, np.float64) for e in traj.extraV_traj]),
        "volume_traj": np.stack([np.asarray(v, np.float64) for v in traj.volume_traj]),
        "grain_size": grain_size, "d_mu": np.float64(d_mu), "d_std": np.float64(d_std),
        "hist_density": dis, "hist_counts": counts.astype(np.int64), "bin_edges": bin_edge.astype(np.float64),
        "patch_size": np.float64(traj.patch_size), "mesh_size": np.float64(traj.mesh_size),
        "ini_height": np.float64(traj.ini_height), "final_height": np.float64(traj.final_height),
        "frames": np.int64(traj.frames), "span": np.int64(SPAN), "lxd": np.float64(traj.lxd),
        "num_regions": np.int64(traj.num_regions), "steps": np.int64(len(rec.xg) - 1),
    }
    path = os.path.join(HERE, out_name)
    np.savez_compressed(path, **out)
    print(f"wrote {out_name}: {os.path.getsize(path)} bytes, {n} grains, {len(rec.xg) - 1} steps, live at the end "
          f"{int(rec.mask[-1].sum())}, d_mu {d_mu:.6f} d_std {d_std:.6f}, counts {counts.tolist()}, "
          f"NaN volumes {int(np.isnan(out['volume_traj']).sum())}")


def load_cfg1():
    import dill
    g40, x, ei, ea = mg.load_graph(os.path.join(mg.REF, "graphs/40_40/seed10020_G1.904_R0.558_span6.pkl"))
    R, Cm = mg.build_reference(mg.make_hyper(g40), x, ei, ea, 10020, 1.0)
    R.threshold, Cm.threshold = 1e-4, 0.6                            # test.py:187-188
    mask = {k: torch.from_numpy(np.asarray(v).astype(np.int64)) for k, v in g40.mask.items()}
    mask["joint"] = 1 + 0 * mask["joint"]                            # test.py:291
    with gzip.open(os.path.join(mg.REF, "graphs/40_40/traj10020.pkl.gz"), "rb") as f:
        traj = dill.load(f)
    traj.raise_err = False
    return traj, R, Cm, x, ei, ea, mask


@torch.no_grad()
def cfg1(events, steps, out_name):
    traj, R, Cm, x, ei, ea, mask = load_cfg1()
    rec = Recorder(traj)
    X, EI, EA = mg.tt(x), mg.tt(ei), mg.tt(ea)
    M = {k: v.clone() for k, v in mask.items()}
    traj.extraV_traj = []                                            # test.py:294
    traj.GNN_update(0, {k: v.clone() for k, v in X.items()}, M, True, EI, False)   # :297
    traj.area_traj = traj.area_traj[:1]                              # :340
    for step in range(1, steps + 1):
        if events:
            pred, gs = mge.step_to_update_point(R, Cm, X, EI, EA, M)
            X, EI, pairs = Cm.update(X, EI, EA, pred, M, gs, 0.0)
            topo = len(pred["grain_event"]) > 0 or len(pairs) > 0
            traj.GNN_update(step * SPAN, {k: v.clone() for k, v in X.items()}, M, topo, EI, False)   # :478
            for grain, coor in traj.region_center.items():           # :556-559
                X["grain"][grain - 1, :2] = torch.FloatTensor(coor)
            print(f"{out_name} step {step}: {len(pred['grain_event'])} grain events, {len(pairs)} switches")
        else:                                                        # make_golden.generate (4): static topology
            pred = R(X, EI, EA)
            pred.update(Cm(X, EI, EA))
            R.update(X, pred, {})
            X["grain"][:, 2] += SPAN / 121
            X["joint"][:, 2] += SPAN / 121
            if X["grain"][0, 2] > 120 / 121:
                X["grain"][:, 2] = 120 / 121
                X["joint"][:, 2] = 120 / 121
            traj.GNN_update(step * SPAN, {k: v.clone() for k, v in X.items()}, M, False, EI, False)
        EA = mge.refresh_edges(X, EI)
    finish(traj, rec, out_name)


def noflux(out_name):
    """make_golden_noflux.run's own loop on its own trajectory object; its fixture file is not rewritten."""
    import graph_trajectory as gt
    import make_golden_noflux as mgn
    made, ctor, save = [], gt.graph_trajectory, np.savez_compressed

    def recording(*a, **kw):
        traj = ctor(*a, **kw)
        made.append((traj, Recorder(traj)))
        return traj
    gt.graph_trajectory, np.savez_compressed = recording, lambda *a, **kw: None
    try:
        mgn.run(40, 1, 10020, "noflux_40_seed1.npz", area_threshold=-0.0065, edge_threshold=0.46418)
    finally:
        gt.graph_trajectory, np.savez_compressed = ctor, save
    traj, rec = made[0]
    # that loop appends the pixel counts, then frame 0, then the steps; test.py:340 keeps the pixel counts as layer 0
    traj.area_traj = traj.area_traj[:1] + traj.area_traj[2:]
    finish(traj, rec, out_name)


if __name__ == "__main__":
    import __main__
    import graph_trajectory as gt
    __main__.graph_trajectory, __main__.graph = gt.graph_trajectory, gt.graph
    cfg1(True, 5, "qoi_cfg1_events.npz")   # (the reference's own update asserts at step 6 of this trajectory)
    cfg1(False, 20, "qoi_cfg1_static.npz")
    noflux("qoi_noflux_40_seed1.npz")
