#!/usr/bin/env python3
"""A/B of the no-flux boundary's cost per rollout step: GrainRollout(boundary="noflux") against boundary="periodic" on the
same structure (tests/golden/noflux_80_seed3.npz: 400 grains, 798 junctions, folded by 2), seeded weights, grain centres
refreshed.  Two loops, each timed after a warm-up, the arms interleaved per repetition:
  run      run() replayed from hipGraphs (the static-topology loop)
  events   run_events() with thresholds no grain or edge reaches (every step quiet: the speculative event loop)
    python tools/noflux_ab.py [--steps 400] [--reps 5]
Prints one line per (loop, arm) with the median and the spread of the per-step time."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from helpers import EDGE_TYPES, GOLDEN, etk, product_models  # noqa: E402
from graingraphnn_amd import GrainRollout  # noqa: E402


def make(d, boundary, R, Cm):
    tt = lambda v: torch.from_numpy(np.array(v, copy=True, order="C")).cuda()
    X = {"grain": tt(d["scaled_x_grain"]), "joint": tt(d["scaled_x_joint"])}
    EI = {et: tt(d["ei_" + etk(et)]) for et in EDGE_TYPES}
    EA = {et: tt(d["scaled_ea_" + etk(et)].reshape(-1, 1)) for et in EDGE_TYPES}
    f = float(d["domain_factor"])
    return GrainRollout(R, Cm, X, EI, EA, int(d["span"]), use_graph=True, refresh_centres=True, domain_factor=f,
                        domain_offset=tt(d["domain_offset"]) if f > 1 else None, boundary=boundary)


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--arms", default="periodic,noflux", help="one arm alone: a kernel trace of it")
    ap.add_argument("--loops", default="run,events")
    a = ap.parse_args()
    arms, loops = a.arms.split(","), a.loops.split(",")
    d = np.load(os.path.join(GOLDEN, "noflux_80_seed3.npz"))
    R, Cm = product_models(int(d["weight_seed"]), 1.0, "cuda")
    mask = {"grain": d["mask_grain"], "joint": d["mask_joint"]}
    times = {}
    for loop in loops:
        ro = {}
        for bc in arms:
            ro[bc] = make(d, bc, R, Cm)
            if loop == "events":
                ro[bc].enable_events(mask, -1e30, 0.9999)
        for rep in range(a.reps + 1):
            for bc in arms:
                r = ro[bc]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if loop == "run":
                    r.run(a.steps)
                else:
                    ev, sw = r.run_events(a.steps)
                    assert not any(len(e) for e in ev) and not any(len(s) for s in sw)
                torch.cuda.synchronize()
                if rep:   # (rep 0: captures and warm-up)
                    times.setdefault((loop, bc), []).append((time.perf_counter() - t0) / a.steps * 1e6)
    print(f"# {os.path.basename(__file__)}: noflux_80_seed3 (400 grains, 798 junctions, folded by 2), {a.steps} steps x "
          f"{a.reps} reps per arm, interleaved; torch {torch.__version__}, {torch.cuda.get_device_name()}")
    for loop in loops:
        med = {}
        for bc in arms:
            t = np.array(times[(loop, bc)])
            med[bc] = float(np.median(t))
            print(f"{loop:6s} {bc:8s} us/step median {med[bc]:8.2f}  min {t.min():8.2f}  max {t.max():8.2f}")
        if len(med) == 2:
            print(f"{loop:6s} noflux - periodic: {med['noflux'] - med['periodic']:+.2f} us/step")


if __name__ == "__main__":
    main()
