"""Golden trajectories of the no-flux boundary condition (test.py:363-375, 418-422, 446-463, 556-559 with
traj.BC == 'noflux'; graph_datastruct.py:689-708): the UNMODIFIED reference, imported at run time through
tools/oracle_stub, on a structure from its own no-flux generator (graph_trajectory(..., BC='noflux')).

Runs only in the build container (needs /root/reference); writes data only:
    python tests/golden/make_golden_noflux.py
      noflux_40_seed1.npz   40 um, one patch (domain_factor 1)
      noflux_80_seed3.npz   80 um, folded onto 2 x 2 patches (domain_factor 2: the offset round trip)

Per fixture: the initial structure (x, the three edge lists, edge lengths, mask, domain offset / factor) and, for every
step k = 1..STEPS of the reference's loop with seeded weights (seeding.seeded_state_dict) and real Cmodel.update events,
`s<k>_*`: both models' predictions, the grain-event list after grain 0 is dropped, the switched pairs, and x / edge lists /
masks / edge lengths after the step.  Step 1 also keeps the forward's filtered lists (`s1_fwd_ei_*`) and the junctions
right after the boundary step (`s1_bnd_x_joint`).
"""
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (sets up sys.path for the reference + stubs)
import numpy as np  # noqa: E402
import torch  # noqa: E402

GJ, JG, JJ = mg.GJ, mg.JG, mg.JJ
SPAN = 6
STEPS = 6
ref_move_to_boundary = mg.ref_function("test.py", "move_to_boundary")


def key(et):
    return "__".join(et)


def forward_edges(EI, EA):
    """test.py:363-375."""
    ei, ea = dict(EI), dict(EA)
    for et, index in EI.items():
        if et[0] == "grain":
            keep = (index[0] > 0).nonzero().view(-1)
            ei[et], ea[et] = index[:, keep], EA[et][keep]
        if et[-1] == "grain":
            keep = (index[1] > 0).nonzero().view(-1)
            ei[et], ea[et] = index[:, keep], EA[et][keep]
    return ei, ea


def refresh_edges(X, EI):
    EA = {}
    for et, index in EI.items():                                    # test.py:562-575
        rel = X[et[0]][index[0], :2] - X[et[-1]][index[-1], :2]
        rel = -1 * (rel > 0.5) + 1 * (rel < -0.5) + rel
        EA[et] = torch.sqrt(rel[:, 0] ** 2 + rel[:, 1] ** 2).view(-1, 1)
    return EA


@torch.no_grad()
def run(lxd, seed, wseed, out_name, G=2.0, R=0.5, area_threshold=1e-4, edge_threshold=0.6):
    import graph_trajectory as gt
    traj = gt.graph_trajectory(lxd=lxd, seed=seed, frames=121, BC="noflux",
                                physical_params={"G": G, "R": R})
    cur_grain, counts = np.unique(traj.alpha_field, return_counts=True)
    traj.area_counts = dict(zip(cur_grain, counts))
    traj.area_traj.append(traj.area_counts)
    traj.form_states_tensor(0)
    hg0 = traj.states[0]
    hg0.span = SPAN
    hg0.form_gradient(prev=None, nxt=None, event_list=None, elim_list=None)
    hg0.append_history([])
    x = {k: np.asarray(v).astype(np.float32) for k, v in hg0.feature_dicts.items()}
    ei = {k: np.asarray(v).astype(np.int64) for k, v in hg0.edge_index_dicts.items()}
    ea = {k: np.asarray(v).astype(np.float32) for k, v in hg0.edge_weight_dicts.items()}
    mask = {k: torch.from_numpy(np.asarray(v).astype(np.int64)) for k, v in hg0.mask.items()}
    mask["joint"] = 1 + 0 * mask["joint"]                              # test.py:258
    out = {"x_grain": x["grain"], "x_joint": x["joint"], "mask_grain": mask["grain"].numpy().copy(),
           "mask_joint": mask["joint"].numpy().copy(), "span": np.int64(SPAN), "lxd": np.int64(lxd),
           "max_y": np.float32(1.0), "area_threshold": np.float32(area_threshold),
           "edge_threshold": np.float32(edge_threshold), "weight_seed": np.int64(wseed)}
    for et in (GJ, JG, JJ):
        out["ei_" + key(et)], out["ea_" + key(et)] = ei[et], ea[et]

    hp = mg.make_hyper(hg0)
    Rm, Cm = mg.build_reference(hp, x, ei, ea, wseed, 1.0)
    Rm.threshold, Cm.threshold = area_threshold, edge_threshold

    X, EI, EA = mg.tt(x), mg.tt(ei), {k: torch.from_numpy(v.copy()).view(-1, 1) for k, v in ea.items()}
    M = {k: v.clone() for k, v in mask.items()}
    gs = {"domain_offset": 0, "domain_factor": traj.lxd / traj.patch_size}  # test.py:310-312
    if gs["domain_factor"] > 1:
        gs["domain_offset"], gs["grain_coor_offset"] = mg.ref_scale_feature_patchs(gs["domain_factor"], X, EA, "noflux")
    out["domain_factor"] = np.float32(gs["domain_factor"])
    out["domain_offset"] = (gs["domain_offset"].numpy().copy() if torch.is_tensor(gs["domain_offset"])
                            else np.zeros((x["joint"].shape[0], 2), np.float32))
    out["scaled_x_grain"], out["scaled_x_joint"] = X["grain"].numpy().copy(), X["joint"].numpy().copy()
    for et in (GJ, JG, JJ):
        out["scaled_ea_" + key(et)] = EA[et].numpy().reshape(-1).copy()
    traj.raise_err = False
    traj.extraV_traj = []
    X0 = {k: v.clone() for k, v in X.items()}
    if gs["domain_factor"] > 1:
        X0["joint"][:, :2] = (X0["joint"][:, :2] + gs["domain_offset"]) / gs["domain_factor"]
    traj.GNN_update(0, X0, M, True, EI, False)                       # test.py:296

    for step in range(1, STEPS + 1):
        s = f"s{step}_"
        EIf, EAf = forward_edges(EI, EA)                              # test.py:363-375
        if step == 1:
            for et in (GJ, JG, JJ):
                out[s + "fwd_ei_" + key(et)] = EIf[et].numpy().copy()
        pred = Rm(X, EIf, EAf)
        pred.update(Cm(X, EIf, EAf))
        for k in ("joint", "grain", "grain_area", "edge_event", "edge"):
            out[s + "pred_" + k] = pred[k].numpy().copy()
        Rm.update(X, pred, gs)
        X["grain"][:, 2] += SPAN / 121
        X["joint"][:, 2] += SPAN / 121
        if X["grain"][0, 2] > 120 / 121:
            X["grain"][:, 2] = 120 / 121
            X["joint"][:, 2] = 120 / 121
        ge = ((M["grain"][:, 0] > 0) & (pred["grain_area"] < Rm.threshold)).nonzero().view(-1)
        ge = ge[torch.argsort(pred["grain_area"][ge])]
        pred["grain_event"] = ge[ge != 0]                             # test.py:421-422
        X, EI, pairs = Cm.update(X, EI, EA, pred, M, gs, 0.0)
        # test.py:446-466
        X["grain"][0, :2] = 0.5
        X["grain"][0, 3:5] = 0
        X["grain"][0, -1] = 0
        X["joint"][:, :2] = (X["joint"][:, :2] + gs["domain_offset"]) / gs["domain_factor"]
        ref_move_to_boundary(X["joint"], EI[GJ], [1, 1])
        X["joint"][:, 0] = torch.clamp(X["joint"][:, 0], min=0, max=1)
        X["joint"][:, 1] = torch.clamp(X["joint"][:, 1], min=0, max=1)
        X["joint"][:, :2] = X["joint"][:, :2] * gs["domain_factor"] - gs["domain_offset"]
        if step == 1:
            out[s + "bnd_x_joint"] = X["joint"].numpy().copy()
        topo = len(pred["grain_event"]) > 0 or len(pairs) > 0
        Xc = {k: v.clone() for k, v in X.items()}
        if gs["domain_factor"] > 1:
            Xc["joint"][:, :2] = (Xc["joint"][:, :2] + gs["domain_offset"]) / gs["domain_factor"]
        traj.GNN_update(step * SPAN, Xc, M, topo, EI, False)
        for grain, coor in traj.region_center.items():               # test.py:556-559
            X["grain"][grain - 1, :2] = torch.FloatTensor(coor)
            if gs["domain_factor"] > 1:
                X["grain"][grain - 1, :2] = (X["grain"][grain - 1, :2] * gs["domain_factor"]) % 1
        EA = refresh_edges(X, EI)
        out[s + "grain_event"] = pred["grain_event"].numpy().astype(np.int64).copy()
        out[s + "switching_list"] = np.asarray(pairs.numpy() if torch.is_tensor(pairs) else pairs).reshape(-1, 2).astype(np.int64)
        out[s + "x_grain"], out[s + "x_joint"] = X["grain"].numpy().copy(), X["joint"].numpy().copy()
        out[s + "mask_grain"], out[s + "mask_joint"] = M["grain"].numpy().copy(), M["joint"].numpy().copy()
        for et in (GJ, JG, JJ):
            out[s + "ei_" + key(et)] = EI[et].numpy().copy()
            out[s + "ea_" + key(et)] = EA[et].numpy().reshape(-1).copy()
        print(f"{out_name} step {step}: {len(out[s + 'grain_event'])} grain events, {len(out[s + 'switching_list'])} switches, "
              f"E_jj {EI[JJ].shape[1]}, grain0 area pred {float(pred['grain_area'][0]):.3g}")
    out["steps"] = np.int64(STEPS)
    np.savez_compressed(os.path.join(HERE, out_name), **out)
    print("wrote", out_name, len(out), "arrays,", os.path.getsize(os.path.join(HERE, out_name)), "bytes;",
          "grains", x["grain"].shape[0], "junctions", x["joint"].shape[0], "factor", gs["domain_factor"])


if __name__ == "__main__":
    import __main__
    import graph_trajectory as gt
    __main__.graph_trajectory, __main__.graph = gt.graph_trajectory, gt.graph
    # thresholds placed between the seeded models' predictions: quiet steps first, then eliminations and switches
    run(40, 1, 10020, "noflux_40_seed1.npz", area_threshold=-0.0065, edge_threshold=0.46418)
    run(80, 3, 10021, "noflux_80_seed3.npz", area_threshold=0.0005, edge_threshold=0.5410)
