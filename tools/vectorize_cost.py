#!/usr/bin/env python3
"""Cost of vectorising a grain-ID image (graingraphnn_amd/vectorize.py) on the benchmark's structure: bench.py's cfg3 (10 000
grains, 20 000 junctions), layer 0 filled into a 4 096 x 4 096 image (67 MB of int32) by GrainRollout.grain_image, then
  counts     ggnn_image_compare                 the per-grain pixel counts: the image read once, the floor
  junctions  ggnn_image_junctions               memset + count pass, scan, emit pass
  links      ggnn_junction_links                the joint->joint columns
  launches   every launch of graph_from_image   counts, junctions, the joint->grain table, links, and their allocations
timed by events per call, median of the rounds after three warm-up rounds.
--boundary noflux times the no-flux mode on the same image cut open at its seams: every id moved up by one (id 1 is the
boundary grain) and the image read with walls.  The benchmark's generator makes periodic structures only, so the grains the
seams cut touch two walls and the status reports their open pairs; the work -- the windows, the wall junctions in grain 0's
row of the table, the links that walk it -- is that of a no-flux structure of this size.
    python tools/vectorize_cost.py [--rounds 50] [--size 4096] [--boundary periodic|noflux]"""
import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--boundary", choices=("periodic", "noflux"), default="periodic")
    a = ap.parse_args()
    sys.path[:0] = [os.path.dirname(HERE)]
    import numpy as np
    import torch
    import bench
    from graingraphnn_amd import GrainRollout, _lib
    from graingraphnn_amd import vectorize as vz
    from graingraphnn_amd.backend import default_backend
    with torch.no_grad():
        R, Cm, X, EI, EA, inputs = bench.build(torch.device("cuda", 0), seed=0)
        ro = GrainRollout(R, Cm, X, EI, EA, bench.SPAN, use_graph=True, refresh_centres=True, domain_factor=inputs[3],
                          domain_offset=torch.from_numpy(inputs[4]))
        ro.enable_polygons(capacity=0)
        image = ro.grain_image((a.size, a.size)).clone()
        n_grain = ro.n_nodes["grain"]
        del ro
        if a.boundary == "noflux":
            image, n_grain = torch.where(image > 0, image + 1, image), n_grain + 1
        v = vz._vectorize(image, n_grain, "cells", 2, None, a.boundary)
        status = dict(zip(vz.STATUS_WORDS, v["status"].tolist()))
        print(f"# {a.boundary} image {tuple(image.shape)} ({image.numel() * 4 / 1e6:.1f} MB), {n_grain} grains, "
              f"{int((image == 0).sum())} uncovered pixels, status {status}, valid {vz.status_is_valid(status, a.boundary)}, "
              f"{int((v['triples'][:status['n_joint'], 0] == 0).sum()) if a.boundary == 'noflux' else 0} wall junctions", flush=True)
        A, L, _, _ = v["calls"]
        lib, be = _lib.load(), default_backend()
        arms = {"counts": lambda: be.image_compare(image, None, n_grain, None, v["counts"]),
                "junctions": lambda: _lib.check(lib.ggnn_image_junctions(ctypes.byref(A), _lib.current_stream()), "junctions"),
                "links": lambda: _lib.check(lib.ggnn_junction_links(ctypes.byref(L), _lib.current_stream()), "links"),
                "launches": lambda: vz._vectorize(image, n_grain, "cells", 2, None, a.boundary)}
        times = {k: [] for k in arms}
        for rnd in range(a.rounds + 3):
            for name, call in arms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call()
                t1.record()
                t1.synchronize()
                if rnd >= 3:
                    times[name].append(t0.elapsed_time(t1) * 1e3)
        for name, t in times.items():
            t = np.array(t)
            print(f"{name:9s} us/call by events: median {np.median(t):8.1f}  min {t.min():8.1f}  max {t.max():8.1f}", flush=True)
        print(f"# torch {torch.__version__}, {torch.cuda.get_device_name()}", flush=True)


if __name__ == "__main__":
    main()
