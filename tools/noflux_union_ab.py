#!/usr/bin/env python3
"""Cost of no-flux ensembles, two measurements:
  boundary   the per-call time of the SINGLE-trajectory boundary launch (ggnn_noflux_boundary on noflux_80_seed3: 798
             junctions, 65 on the walls) of this tree's library against another build of the library (--other-lib: the commit
             before, whose kernel knew one grain 0), interleaved per repetition, with an A/A pair of this tree's library for
             the spread; and ggnn_noflux_boundary_traj on a union of --traj copies beside them
  union      trajectory-steps/s of --traj perturbed 40 um no-flux trajectories (noflux_40_seed1) through --steps
             step_events() as ONE union (GrainRollout(boundary="noflux", traj_offsets=...)) against the same rollouts one
             after another
    python tools/noflux_union_ab.py [--traj 64] [--steps 6] [--other-lib PATH] [--out profiles/r10_noflux_union.txt]"""
import argparse
import ctypes
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traj", type=int, default=64)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--sigma", type=float, default=2e-3)
    ap.add_argument("--other-lib", default=None, help="a libggnn.so of another commit (the A/B of the boundary launch)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_noflux_union.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from helpers import EDGE_TYPES, GOLDEN, etk, product_models, tt
    from graingraphnn_amd import GrainRollout, _lib, synthetic
    from graingraphnn_amd.backend import default_backend
    from graingraphnn_amd.topology import TopologyError

    dev, sync = "cuda", torch.cuda.synchronize
    GJ, JG, JJ = EDGE_TYPES
    be = default_backend()
    lines = [f"noflux_union_ab: device {torch.cuda.get_device_name(0)}, torch {torch.__version__}"]

    # ---- the boundary launch ----------------------------------------------------------------------------------------
    d = np.load(os.path.join(GOLDEN, "noflux_80_seed3.npz"))
    f, nj, ng = float(d["domain_factor"]), d["x_joint"].shape[0], d["x_grain"].shape[0]
    dv = lambda a: torch.from_numpy(np.array(a, copy=True, order="C")).to(dev)
    xj, xg, off = dv(d["scaled_x_joint"]), dv(d["scaled_x_grain"]), dv(d["domain_offset"])
    csr = be.build_csr(dv(d["ei_" + etk(JG)]), nj, ng)
    single = (_lib.ptr(csr.rowptr), _lib.ptr(csr.col), _lib.ptr(xj), nj, xj.stride(0), _lib.ptr(off), f, 1.0, _lib.ptr(xg),
              xg.stride(0), xg.size(1), None)
    libs = {"this tree (A)": be.lib, "this tree (A')": be.lib}
    if args.other_lib:
        other = ctypes.CDLL(os.path.abspath(args.other_lib))
        other.ggnn_noflux_boundary.restype = ctypes.c_int
        other.ggnn_noflux_boundary.argtypes = be.lib.ggnn_noflux_boundary.argtypes
        libs[f"other build ({os.path.basename(os.path.dirname(os.path.abspath(args.other_lib))) or args.other_lib})"] = other
    T = args.traj
    ogu, oju = dv(np.arange(T + 1, dtype=np.int64) * ng), dv(np.arange(T + 1, dtype=np.int64) * nj)
    jg = d["ei_" + etk(JG)]
    jgu = np.concatenate([jg + np.array([[t * nj], [t * ng]]) for t in range(T)], axis=1)
    csru = be.build_csr(dv(jgu), T * nj, T * ng)
    xju, xgu, offu = xj.repeat(T, 1), xg.repeat(T, 1), off.repeat(T, 1)
    union = (_lib.ptr(csru.rowptr), _lib.ptr(csru.col), _lib.ptr(xju), T * nj, xju.stride(0), _lib.ptr(offu), f, 1.0,
             _lib.ptr(xgu), xgu.stride(0), xgu.size(1), None, _lib.ptr(ogu), _lib.ptr(oju), T)
    calls = {name: (lambda lib=lib: lib.ggnn_noflux_boundary(*single, _lib.current_stream())) for name, lib in libs.items()}
    calls[f"ggnn_noflux_boundary_traj, {T} trajectories ({T * nj} junctions)"] = \
        lambda: be.lib.ggnn_noflux_boundary_traj(*union, _lib.current_stream())
    n, reps, times = 500, 7, {k: [] for k in calls}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(reps + 1):
        for name, call in calls.items():   # (interleaved: every repetition visits every arm)
            a.record()
            for _ in range(n):
                assert call() == 0
            b.record()
            sync()
            if rep:
                times[name].append(a.elapsed_time(b) * 1e3 / n)
    lines.append(f"boundary launch, noflux_80_seed3 ({nj} junctions, folded by {f:g}); {n} calls back to back, {reps} repetitions, "
                 "arms interleaved; us per call")
    for name, t in times.items():
        lines.append(f"  {name:58s} median {np.median(t):6.2f}  min {min(t):6.2f}  max {max(t):6.2f}")

    # ---- the ensemble -------------------------------------------------------------------------------------------------
    d = np.load(os.path.join(GOLDEN, "noflux_40_seed1.npz"))
    base = {"grain": d["scaled_x_grain"], "joint": d["scaled_x_joint"]}
    ei = {et: d["ei_" + etk(et)] for et in EDGE_TYPES}
    ea = {et: d["scaled_ea_" + etk(et)].reshape(-1, 1) for et in EDGE_TYPES}
    graphs = [(synthetic.perturbed_copy(base, args.sigma, 1000 + t), ei, ea) for t in range(T)]
    R, Cm = product_models(int(d["weight_seed"]), 1.0, dev)
    thr = (float(d["area_threshold"]), float(d["edge_threshold"]))
    kw = dict(use_graph=True, refresh_centres=True, boundary="noflux", max_y=float(d["max_y"]))

    def rollout(gs, union=False):
        x, e, w, slices = synthetic.disjoint_union(gs)
        off = {nt: [s[nt][0] for s in slices] + [slices[-1][nt][1]] for nt in ("grain", "joint")}
        ro = GrainRollout(R, Cm, tt(x, dev), tt(e, dev), tt(w, dev), int(d["span"]), **kw, **({"traj_offsets": off} if union else {}))
        ro.enable_events({k: np.concatenate([d["mask_" + k]] * len(gs)) for k in ("grain", "joint")}, *thr)
        return ro

    def to_its_end(ro):
        for _ in range(args.steps):
            try:
                ro.step_events()
            except TopologyError:
                break
        return ro.steps_done

    with torch.no_grad():
        to_its_end(rollout(graphs[:1]))   # warm-up
        sync()
        t_build = t_loop = 0.0
        ends = []
        for g in graphs:
            t0 = time.perf_counter()
            ro = rollout([g])
            sync()
            t1 = time.perf_counter()
            ends.append(to_its_end(ro))
            sync()
            t2 = time.perf_counter()
            t_build, t_loop = t_build + t1 - t0, t_loop + t2 - t1
        done = sum(ends)
        lines += [f"ensemble: {T} perturbed noflux_40_seed1 trajectories (sigma {args.sigma:g}), at most {args.steps} steps each",
                  f"  sequential: {done} trajectory-steps in {t_loop:.3f} s = {done / t_loop:.0f} trajectory-steps/s "
                  f"(+ {t_build:.3f} s constructing the {T} rollouts)"]
        for rep in ("warm-up", "timed"):
            t0 = time.perf_counter()
            ro = rollout(graphs, union=True)
            sync()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                ro.step_events()
            sync()
            t2 = time.perf_counter()
        got = [args.steps if e_ is None else e_ for e_ in ro._ens["ended_at"]]
        lines += [f"  union: {sum(got)} trajectory-steps in {t2 - t1:.3f} s = {sum(got) / (t2 - t1):.0f} trajectory-steps/s "
                  f"(+ {t1 - t0:.3f} s constructing the union rollout)",
                  f"  union and sequential end steps agree: {got == ends}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
