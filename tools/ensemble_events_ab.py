#!/usr/bin/env python3
"""Event-driven ensemble: 64 perturbed copies of the 40 um fixture (cfg1: 118 grains, 236 junctions each), every one run
through step_events() to ITS end -- the step at which its topology update is refused -- or to --max-steps:
  sequential  64 GrainRollouts one after another, enable_events(mask, ...) each: what a user had before events per trajectory
  union       ONE GrainRollout on the disjoint union, enable_events(mask, ..., traj_offsets=...): a refused trajectory ends,
              the others go on (only where the tree under --root has it)
Both report trajectory-steps per second of the step loops (construction and graph capture apart, reported beside).  The
per-call time of the two detection entry points (memset + kernel, back to back on one stream, cuda events) is measured on the
union's own buffers.  --root DIR: run the arms against another checkout (the parent commit with its library built) for the
sequential arm there.
    python tools/ensemble_events_ab.py [--traj 64] [--max-steps 40] [--root DIR] [--out profiles/r9_ensemble_events.txt]"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traj", type=int, default=64)
    ap.add_argument("--max-steps", type=int, default=40)
    ap.add_argument("--sigma", type=float, default=1e-3)
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "r9_ensemble_events.txt"))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import numpy as np
    import torch
    from helpers import load_graph, product_models, tt
    from graingraphnn_amd import GrainRollout, synthetic
    from graingraphnn_amd.topology import TopologyError

    dev = "cuda"
    x, ei, ea = load_graph("40")
    graphs = [(synthetic.perturbed_copy(x, args.sigma, 1000 + t), ei, ea) for t in range(args.traj)]
    R, Cm = product_models(10020, 1.0, dev)
    lines = [f"ensemble_events_ab: {args.traj} perturbed cfg1 trajectories (sigma {args.sigma:g}), at most {args.max_steps} steps each, "
             f"tree {root}", f"device: {torch.cuda.get_device_name(0)}"]
    sync = torch.cuda.synchronize

    def own_rollout(g):
        ro = GrainRollout(R, Cm, tt(g[0], dev), tt(g[1], dev), tt(g[2], dev), 6, use_graph=True, refresh_centres=True)
        ro.enable_events({"grain": np.ones((118, 1)), "joint": np.ones((236, 1))}, 1e-4, 0.6)
        return ro

    def to_its_end(ro):
        for _ in range(args.max_steps):
            try:
                ro.step_events()
            except TopologyError:
                break
        return ro.steps_done

    with torch.no_grad():
        to_its_end(own_rollout(graphs[0]))   # warm-up: library, allocator, first captures
        sync()
        t_build = t_loop = 0.0
        ends = []
        for g in graphs:
            t0 = time.perf_counter()
            ro = own_rollout(g)
            sync()
            t1 = time.perf_counter()
            ends.append(to_its_end(ro))
            sync()
            t2 = time.perf_counter()
            t_build, t_loop = t_build + t1 - t0, t_loop + t2 - t1
        done = sum(ends)
        lines += [f"completed steps per trajectory: min {min(ends)}, max {max(ends)}, total {done}",
                  f"sequential: {done} trajectory-steps in {t_loop:.3f} s = {done / t_loop:.0f} trajectory-steps/s "
                  f"(+ {t_build:.3f} s constructing the {args.traj} rollouts)"]
        if hasattr(GrainRollout, "trajectory_states"):
            xu, eiu, eau, slices = synthetic.disjoint_union(graphs)
            off = {nt: [s[nt][0] for s in slices] + [slices[-1][nt][1]] for nt in ("grain", "joint")}
            for rep in ("warm-up", "timed"):
                t0 = time.perf_counter()
                ro = GrainRollout(R, Cm, tt(xu, dev), tt(eiu, dev), tt(eau, dev), 6, use_graph=True, refresh_centres=True)
                ro.enable_events({"grain": np.ones((off["grain"][-1], 1)), "joint": np.ones((off["joint"][-1], 1))}, 1e-4, 0.6,
                                 traj_offsets=off)
                sync()
                t1 = time.perf_counter()
                steps = 0
                while steps < args.max_steps and any(e is None for e in ro._ens["ended_at"]):
                    ro.step_events()
                    steps += 1
                sync()
                t2 = time.perf_counter()
            got = [steps if e is None else e for e in ro._ens["ended_at"]]
            lines += [f"union: {sum(got)} trajectory-steps in {t2 - t1:.3f} s = {sum(got) / (t2 - t1):.0f} trajectory-steps/s, "
                      f"{steps} union steps (+ {t1 - t0:.3f} s constructing the union rollout)",
                      f"union and sequential end steps agree: {got == ends}"]
            # the two detection entry points on the union's buffers, as step_events() calls them
            E, p, be = ro._ens, ro.pred, ro.be
            flags = torch.zeros(2, dtype=torch.int32, device=dev)
            calls = {
                "ggnn_detect_events (detect_events_kernel<false>)": lambda: be.detect_events(
                    p["grain_area"], ro._live_grain, ro.area_threshold, p["edge_event"], ro.graph.edge_index[("joint", "connect", "joint")],
                    ro._logit_trigger, flags),
                "ggnn_detect_events_traj (detect_events_kernel<true>)": lambda: be.detect_events_traj(
                    p["grain_area"], ro._live_grain, ro.area_threshold, p["edge_event"], ro.graph.edge_index[("joint", "connect", "joint")],
                    ro._logit_trigger, E["grain_off"], E["joint_off"], ro._ev_flags[2:], ro._ev_flags[:2], ended=E["ended"])}
            n = 500
            for name, call in calls.items():
                for _ in range(50):
                    call()
                sync()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                best = None
                for _ in range(5):
                    a.record()
                    for _ in range(n):
                        call()
                    b.record()
                    sync()
                    us = a.elapsed_time(b) * 1e3 / n
                    best = us if best is None else min(best, us)
                lines.append(f"{name}: {best:.2f} us per call (memset + kernel, {n} back to back, best of 5; "
                             f"{ro.n_nodes['grain']} grains, {ro.edge_index[('joint', 'connect', 'joint')].size(1)} junction edges)")
        else:
            lines.append("union: this tree has no events per trajectory")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
