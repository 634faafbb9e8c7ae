#!/usr/bin/env python3
"""Cost of the polygon recorder per rollout step on the benchmark's workload (bench.py's cfg3: 10 000 grains, 20 000
junctions, two-stream plan, run() replayed from hipGraphs of 10 steps, grain centres refreshed).  Arms, interleaved per
repetition inside one process, each timed after a warm-up repetition:
  off   enable_polygons not called
  on    enable_polygons(capacity=RING): the arena holds RING layers beyond layer 0 and the layer word is set back to 0
        between repetitions, so that a long timing does not need an arena of thousands of layers
With --parent-root DIR (a checkout of the parent commit with its library built) the same loop runs there as an A/A pair
`parent_a` / `parent_b` in a process of its own, before and after this tree's: the spread between the two is the yardstick
for `off`.
    python tools/polygons_ab.py [--steps 500] [--reps 5] [--parent-root DIR] [--out FILE]
--kernel N: nothing but N launches of ggnn_grain_polygons on the benchmark's state (for a kernel trace run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/polygons_ab.py --kernel 200)"""
import argparse
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def build(root):
    sys.path[:0] = [root]
    import torch
    import bench
    from graingraphnn_amd import GrainRollout
    R, Cm, X, EI, EA, inputs = bench.build(torch.device("cuda", 0), seed=0)

    def rollout():
        Xa = {k: v.clone() for k, v in X.items()}
        return GrainRollout(R, Cm, Xa, EI, EA, bench.SPAN, use_graph=True, refresh_centres=True, domain_factor=inputs[3],
                            domain_offset=torch.from_numpy(inputs[4]))
    return rollout


def worker(root, arms, steps, reps):
    import numpy as np
    import torch
    with torch.no_grad():
        rollout = build(root)
        ro = {arm: rollout() for arm in arms}
        for arm in arms:
            if arm == "on":
                ro[arm].enable_polygons(capacity=steps)
        times = {arm: [] for arm in arms}
        for rep in range(reps + 1):
            for arm in arms:
                if arm == "on":   # the arena's rows are written again
                    ro[arm]._carry_home()
                    ro[arm]._poly["home"]["flat"].zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ro[arm].run(steps)
                torch.cuda.synchronize()
                if rep:   # (rep 0: captures and warm-up)
                    times[arm].append((time.perf_counter() - t0) / steps * 1e6)
        for arm in arms:
            if arm == "on":
                p = ro[arm].polygons()
                assert p["layers"] == steps
                print(f"# recorded {steps} layers of {p['sides'].numel()} grains, sides {int(p['sides'].min())}-"
                      f"{int(p['sides'].max())}, {int(p['rowptr'][-1])} table entries", flush=True)
            t = np.array(times[arm])
            print(f"{arm:10s} us/step median {np.median(t):8.2f}  min {t.min():8.2f}  max {t.max():8.2f}  "
                  f"steps/s {1e6 / np.median(t):8.1f}", flush=True)
        print(f"# torch {torch.__version__}, {torch.cuda.get_device_name()}", flush=True)


def kernel_only(root, n):
    import torch
    with torch.no_grad():
        ro = build(root)()
        ro.run(10)
        JG = ("joint", "pull", "grain")
        arena = None
        for _ in range(n):
            arena = ro.be.grain_polygons(ro.graph.csr_full[JG], ro.x["joint"], arena, ro.domain_factor, ro.domain_offset)
        torch.cuda.synchronize()
        sides = arena["rowptr"][0, 1:] - arena["rowptr"][0, :-1]
        print(f"{n} launches: {sides.numel()} grains, {int(arena['rowptr'][0, -1])} table entries, sides {int(sides.min())}-"
              f"{int(sides.max())}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel", type=int, default=0)
    ap.add_argument("--worker", nargs=2, metavar=("ROOT", "ARMS"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(os.path.abspath(a.worker[0]), a.worker[1].split(","), a.steps, a.reps)
    root = os.path.dirname(HERE)
    if a.kernel:
        return kernel_only(root, a.kernel)
    runs = [("this tree", root, "off,on")]
    if a.parent_root:
        parent = ("parent commit", a.parent_root, "parent_a,parent_b")
        runs = [parent, runs[0], parent]
    lines = [f"# {os.path.basename(__file__)}: cfg3 (10000 grains, 20000 junctions), run() from hipGraphs, {a.steps} steps x {a.reps} "
             "reps per arm, arms interleaved per repetition, one process per block below"]
    for what, where, arms in runs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--reps", str(a.reps),
                            "--worker", where, arms], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit(f"{what}: worker failed\n{r.stdout[-2000:]}{r.stderr[-3000:]}")
        lines += [f"## {what}"] + [ln for ln in r.stdout.splitlines() if ln.strip()]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
