#!/usr/bin/env python3
"""Cost of the grain-ID image on the benchmark's state (bench.py's cfg3: 10 000 grains, 20 000 junctions; layer 0 of the
polygon recorder; image 4 601 x 4 601 = 85 MB of int32).  N rounds of, on one stream,
  image   GrainRollout.grain_image(size, out=image)      the call's own zeroing (a memset) + ggnn_polygons_rasterize's kernel
  fill    other.fill_(7)                                 a plain fill of an image of the same size: the floor
  error   GrainRollout.image_error(image, other)         ggnn_image_compare
timed by events per call, and meant for a kernel trace run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/raster_cost.py --rounds 200
    python tools/raster_cost.py [--rounds 200] [--size 4601]"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--size", type=int, default=4601)
    a = ap.parse_args()
    sys.path[:0] = [os.path.dirname(HERE)]
    import numpy as np
    import torch
    import bench
    from graingraphnn_amd import GrainRollout
    with torch.no_grad():
        R, Cm, X, EI, EA, inputs = bench.build(torch.device("cuda", 0), seed=0)
        ro = GrainRollout(R, Cm, X, EI, EA, bench.SPAN, use_graph=True, refresh_centres=True, domain_factor=inputs[3],
                          domain_offset=torch.from_numpy(inputs[4]))
        ro.enable_polygons(capacity=0)
        size = (a.size, a.size)
        image = ro.grain_image(size)
        other = torch.empty_like(image)
        p = ro.polygons()
        box = (p["xy_sorted"] * a.size).int()
        print(f"# {p['sides'].numel()} polygons, sides {int(p['sides'].min())}-{int(p['sides'].max())}, image {tuple(image.shape)} "
              f"({image.numel() * 4 / 1e6:.1f} MB), {int((image == 0).sum())} uncovered pixels, vertex pixels "
              f"{int(box.min())}..{int(box.max())}", flush=True)
        arms = {"image": lambda: ro.grain_image(size, out=image), "fill": lambda: other.fill_(7),
                "error": lambda: ro.be.image_compare(image, other, ro.n_nodes["grain"])}
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
            print(f"{name:6s} us/call by events: median {np.median(t):8.1f}  min {t.min():8.1f}  max {t.max():8.1f}", flush=True)
        print(f"# torch {torch.__version__}, {torch.cuda.get_device_name()}", flush=True)


if __name__ == "__main__":
    main()
