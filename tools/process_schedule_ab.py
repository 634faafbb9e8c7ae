#!/usr/bin/env python3
"""Cost of the (G, R) schedule on the device on the benchmark's workload (bench.py's cfg3: 10 000 grains, 20 000
junctions, two-stream plan, hipGraphs, grain centres refreshed).  Arms, interleaved per repetition inside one process, each
timed after a warm-up repetition:
  schedule   set_process_schedule(G, R) with --steps rows, then run(--steps): the rows follow the device-side counter
             inside the RUN_UNROLL graphs
  host_loop  what a time-varying rollout had to do before: set_process_parameters(G[k], R[k]) + step(), --steps times
  static     run(--steps), no schedule
and the per-call time of ggnn_process_schedule on the workload's junctions (calls back to back on one stream, between two
events).  With --parent-root DIR (a checkout of the parent commit with its library built) `static` runs there as an A/A
pair `parent_a` / `parent_b` in a process of its own, before and after this tree's: the spread between the two is the
yardstick for what the feature costs when it is off.
    python tools/process_schedule_ab.py [--steps 100] [--reps 7] [--parent-root DIR] [--out profiles/r11_process_schedule.txt]"""
import argparse
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def worker(root, arms, steps, reps):
    sys.path[:0] = [root]
    import numpy as np
    import torch
    import bench
    from graingraphnn_amd import GrainRollout
    rs = np.random.RandomState(0)
    G, Rp = rs.uniform(0.5, 10.0, steps), rs.uniform(0.2, 2.0, steps)
    with torch.no_grad():
        R, Cm, X, EI, EA, inputs = bench.build(torch.device("cuda", 0), seed=0)
        ro = {}
        for arm in arms:
            Xa = {k: v.clone() for k, v in X.items()}
            ro[arm] = GrainRollout(R, Cm, Xa, EI, EA, bench.SPAN, use_graph=True, refresh_centres=True, domain_factor=inputs[3],
                                   domain_offset=torch.from_numpy(inputs[4]))

        def advance(arm):
            if arm == "schedule":
                ro[arm].set_process_schedule(G, Rp)
                ro[arm].run(steps)
            elif arm == "host_loop":
                for k in range(steps):
                    ro[arm].set_process_parameters(G[k], Rp[k])
                    ro[arm].step()
            else:
                ro[arm].run(steps)
        times = {arm: [] for arm in arms}
        for rep in range(reps + 1):
            for arm in arms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                advance(arm)
                torch.cuda.synchronize()
                if rep:   # (rep 0: captures and warm-up)
                    times[arm].append((time.perf_counter() - t0) / steps * 1e6)
        for arm in arms:
            t = np.array(times[arm])
            print(f"{arm:10s} us/step median {np.median(t):8.2f}  min {t.min():8.2f}  max {t.max():8.2f}  "
                  f"steps/s {1e6 / np.median(t):8.1f}", flush=True)
        if "schedule" in arms:
            from graingraphnn_amd.backend import default_backend
            be, S, xj = default_backend(), ro["schedule"]._sched, ro["schedule"].x["joint"]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n, per_call = 500, []
            for rep in range(reps + 1):
                a.record()
                for _ in range(n):
                    be.process_schedule(xj, S["table"], S["offsets"], S["home"]["flat"], S["home"]["flat"], S["sync"])
                b.record()
                torch.cuda.synchronize()
                if rep:
                    per_call.append(a.elapsed_time(b) * 1e3 / n)
            print(f"ggnn_process_schedule, {xj.size(0)} junctions, {n} calls back to back: us per call median "
                  f"{np.median(per_call):6.2f}  min {min(per_call):6.2f}  max {max(per_call):6.2f}", flush=True)
        print(f"# torch {torch.__version__}, {torch.cuda.get_device_name()}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", nargs=2, metavar=("ROOT", "ARMS"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(os.path.abspath(a.worker[0]), a.worker[1].split(","), a.steps, a.reps)
    root = os.path.dirname(HERE)
    runs = [("this tree", root, "schedule,host_loop,static")]
    if a.parent_root:
        parent = ("parent commit", a.parent_root, "parent_a,parent_b")
        runs = [parent, runs[0], parent]
    lines = [f"# {os.path.basename(__file__)}: cfg3 (10000 grains, 20000 junctions), hipGraphs, {a.steps} steps x {a.reps} "
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
