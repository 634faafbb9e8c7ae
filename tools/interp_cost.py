#!/usr/bin/env python3
"""Cost of the in-between layers on the benchmark's workload (bench.py's cfg3: 10 000 grains, 20 000 junctions, two-stream
plan, run() replayed from hipGraphs, grain centres refreshed).  One mode per call:
  --recorder      run(--steps) with the polygon recorder at positions=False (`polygons`) against positions=True
                  (`positions`: ggnn_polygon_inputs in front of every polygon launch), interleaved per repetition inside one
                  process, each timed after a warm-up repetition; the layer word is set back between repetitions
  --kernel N      20 recorded layers, then N calls of ggnn_interp_polygons with --jobs jobs each, timed by events per call,
                  and meant for a kernel trace run of its own:
                      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/interp_cost.py --kernel 100 --jobs 1
  --volume N      20 recorded layers, then N calls of grain_volume(size, interp_frames=2): 61 images, 40 of them in-between,
                  by events per call
    python tools/interp_cost.py --recorder [--steps 500] [--reps 5] | --kernel N [--jobs 1] | --volume N [--size 4601]"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
LAYERS = 20


def build():
    sys.path[:0] = [os.path.dirname(HERE)]
    import torch
    import bench
    from graingraphnn_amd import GrainRollout
    R, Cm, X, EI, EA, inputs = bench.build(torch.device("cuda", 0), seed=0)

    def rollout():
        Xa = {k: v.clone() for k, v in X.items()}
        return GrainRollout(R, Cm, Xa, EI, EA, bench.SPAN, use_graph=True, refresh_centres=True, domain_factor=inputs[3],
                            domain_offset=torch.from_numpy(inputs[4]))
    return rollout


def stats(name, t, unit="us/call"):
    import numpy as np
    t = np.array(t)
    print(f"{name:10s} {unit} median {np.median(t):9.2f}  min {t.min():9.2f}  max {t.max():9.2f}", flush=True)


def recorder(steps, reps):
    import torch
    rollout = build()
    arms = ("polygons", "positions")
    ro = {arm: rollout() for arm in arms}
    for arm in arms:
        ro[arm].enable_polygons(capacity=steps, positions=arm == "positions")
    times = {arm: [] for arm in arms}
    for rep in range(reps + 1):
        for arm in arms:
            ro[arm]._carry_home()
            ro[arm]._poly["home"]["flat"].zero_()   # the arena's rows are written again
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ro[arm].run(steps)
            torch.cuda.synchronize()
            if rep:   # (rep 0: captures and warm-up)
                times[arm].append((time.perf_counter() - t0) / steps * 1e6)
    p = ro["positions"].polygons()
    assert p["layers"] == steps and ro["polygons"].polygons()["layers"] == steps
    moved = (p["col"].numel() * 4 + p["joint_xy"].numel() * 4) * 2
    print(f"# {steps} steps x {reps} reps per arm; per layer {p['col'].numel()} columns and {p['joint_xy'].size(0)} junctions: "
          f"{moved / 1e6:.2f} MB read + written", flush=True)
    for arm in arms:
        stats(arm, times[arm], "us/step")


def recorded():
    ro = build()()
    ro.enable_polygons(capacity=LAYERS, positions=True)
    ro.run(LAYERS)
    assert ro.polygons()["layers"] == LAYERS
    return ro


def by_events(call, n, warm=3):
    import torch
    out = []
    for rnd in range(n + warm):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        if rnd >= warm:
            out.append(t0.elapsed_time(t1) * 1e3)
    return out


def kernel(n, jobs):
    ro = recorded()
    P = ro._poly
    todo = [(1 + i % LAYERS, ((i * 7) % 19 + 1) / 20) for i in range(jobs)]
    out = ro.be.interp_polygons(P["arena"], P["inputs"], todo, LAYERS, ro.boundary, ro.max_y)
    call = lambda: ro.be.interp_polygons(P["arena"], P["inputs"], todo, LAYERS, ro.boundary, ro.max_y, out=out)
    print(f"# {jobs} jobs per call over {LAYERS} recorded layers, {out['rowptr'].size(1) - 1} grains, "
          f"{int(out['rowptr'][0, -1])} table entries; the call allocates its workspace", flush=True)
    stats(f"{jobs} jobs", by_events(call, n))


def volume(n, size):
    import torch
    ro = recorded()
    vol = ro.grain_volume((size, size), interp_frames=2)
    print(f"# volume {tuple(vol.shape)} int32 ({vol.numel() * 4 / 1e9:.2f} GB), {int((vol == 0).sum())} uncovered pixels", flush=True)
    stats("volume", [t / 1e3 for t in by_events(lambda: ro.grain_volume((size, size), interp_frames=2, out=vol), n, warm=1)], "ms/call")
    stats("images", [t / 1e3 for t in by_events(lambda: ro.grain_images((size, size), out=vol[:LAYERS + 1]), n, warm=1)], "ms/call")
    print(f"# torch {torch.__version__}, {torch.cuda.get_device_name()}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recorder", action="store_true")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel", type=int, default=0)
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--volume", type=int, default=0)
    ap.add_argument("--size", type=int, default=4601)
    a = ap.parse_args()
    import torch
    with torch.no_grad():
        if a.recorder:
            recorder(a.steps, a.reps)
        elif a.kernel:
            kernel(a.kernel, a.jobs)
        elif a.volume:
            volume(a.volume, a.size)
        else:
            ap.error("one of --recorder, --kernel N, --volume N")


if __name__ == "__main__":
    main()
