#!/usr/bin/env python3
"""Development aid: what the input gradients cost.  Forward + regressor loss + backward of the HIP training
path, captured in a hipGraph and replayed, once with x_dict / edge_attr as plain data and once with all of them requiring
grad; the two graphs are timed in alternating rounds.  Also the kernels of one eager pass of each kind (torch profiler).

    python tools/input_grad_cost.py [--cfg3] [--batch 4] [--rounds 7] [--replays 20] [--bf16]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graingraphnn_amd import synthetic, training  # noqa: E402
from graingraphnn_amd.models import GrainNN_regressor  # noqa: E402
from graingraphnn_amd.seeding import load_seeded  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg3", action="store_true", help="the 10k-grain honeycomb (default: --batch copies of the 40 um fixture)")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--bf16", action="store_true")
    args = ap.parse_args()
    if args.cfg3:
        x, ei, ea = synthetic.honeycomb(100, 10, 0)
        name = "cfg3 honeycomb (10000 grains)"
    else:
        x0, ei0, ea0 = synthetic.load_fixture(os.path.join(ROOT, "tests", "golden", "graph_40.npz"))
        x, ei, ea, _ = synthetic.disjoint_union([(synthetic.perturbed_copy(x0, 1e-3, 1000 + t), ei0, ea0) for t in range(args.batch)])
        name = f"{args.batch} x 40 um fixture"
    rs = np.random.RandomState(3)
    dev = torch.device("cuda", 0)
    R = load_seeded(GrainNN_regressor(synthetic.default_hyper(dev)), 0, 1.0).to(dev).train()
    Y = {nt: torch.from_numpy(rs.uniform(-1, 1, (x[nt].shape[0], 2)).astype(np.float32)).to(dev) for nt in x}
    M = {nt: torch.ones(x[nt].shape[0], 1, device=dev) for nt in x}

    def make(with_inputs):
        X, EI, EA = synthetic.to_torch(x, ei, ea, dev)
        if with_inputs:
            for d in (X, EA):
                for v in d.values():
                    v.requires_grad_(True)

        def one():
            for p in R.parameters():
                p.grad = None
            for d in (X, EA):
                for v in d.values():
                    v.grad = None
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=args.bf16):
                loss = training.regressor_loss(Y, R(X, EI, EA), M)
            loss.backward()
            return loss
        return one

    graphs, eager = {}, {}
    for kind in (False, True):
        one = eager[kind] = make(kind)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                one()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                one()
        torch.cuda.current_stream().wait_stream(s)
        graphs[kind] = g
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(args.rounds):
        for kind in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            graphs[kind].replay()
            e0.record()
            for _ in range(args.replays):
                graphs[kind].replay()
            e1.record()
            torch.cuda.synchronize()
            ms[kind].append(e0.elapsed_time(e1) / args.replays)
    for kind in (False, True):
        v = ms[kind]
        print(f"{name}{' bf16' if args.bf16 else ''}: forward + loss + backward {'WITH' if kind else 'without'} input gradients: "
              f"median {statistics.median(v):.3f} ms  (min {min(v):.3f}, max {max(v):.3f}; {args.rounds} rounds x {args.replays} replays)")
    print(f"  difference of the medians: {1e3 * (statistics.median(ms[True]) - statistics.median(ms[False])):.0f} us")
    try:
        from torch.profiler import ProfilerActivity, profile
        for kind in (False, True):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                eager[kind]()
                torch.cuda.synchronize()
            names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
            kern = [n for n in names if not n.lower().startswith(("memcpy", "memset"))]
            print(f"  eager pass {'WITH' if kind else 'without'} input gradients: {len(kern)} kernels "
                  f"({sum('ggnn' in n for n in kern)} ggnn), {len(names) - len(kern)} copies / fills")
    except Exception as e:   # (no profiler in this build: the timing above stands)
        print(f"  kernel count unavailable: {type(e).__name__}: {e}")


if __name__ == "__main__":
    main()
