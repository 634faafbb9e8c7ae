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
    python tools/vectorize_cost.py [--rounds 50] [--size 4096] [--boundary periodic|noflux]
--union B times the union path at about bench.py's cfg4 shape instead (cfg4 has 118 grains a trajectory): B images of
--size x --size (128 when not given) with 121 grains each -- Voronoi cells of a jittered brick lattice, made on the device from --seed; candidates that are no valid
structure (an edge below a pixel) are dropped --, and prints
  loop       B x sample_from_image, the results to the host, synthetic.disjoint_union, the union uploaded again: the only
             route before samples_from_images
  union      one samples_from_images
  calls x B  B x (ggnn_image_compare + ggnn_image_junctions + ggnn_junction_links) on prepared arguments
  calls      ggnn_image_junctions_traj + ggnn_junction_links_traj on prepared arguments
loop and union by the host clock around work that ends in a synchronise (both hold host work), the calls by events; median of
the rounds after three warm-up rounds, the arms alternating within a round.  The kernel launches of one loop and of one
union call are counted by torch.profiler in a pass of their own after the timing, which also lists the device time of
every kernel of the two union calls (the count, scan and emit passes by name).
    python tools/vectorize_cost.py --union 64 [--rounds 20] [--boundary periodic]
--track T times the way from a recorded sequence to training samples (vectorize.frames_to_samples): T frames of --size x --size
(128 when not given) with 121 grains, the Voronoi cells of lattice seeds that drift from frame to frame, and prints
  host       the only route before it: graphs_from_images(strict=False), the union's arrays read back, the matcher and the
             targets of the restatement (tests/trackcheck.py) on the host
  samples    one frames_to_samples
  calls      ggnn_track_junctions + ggnn_track_targets on prepared arguments
host and samples by the host clock around work that ends in a synchronise, the calls by events; the same protocol as --union.
The device activities of one frames_to_samples and of the two calls are counted at T = 8 and at T: they must not differ.
    python tools/vectorize_cost.py --track 64 [--rounds 20]
--trace adds linking by tracing boundaries (links="trace", ggnn_junction_links_trace_traj).  On the 4 096 x 4 096 image, read as a
one-image union: ggnn_junction_links_traj and the trace call behind it on prepared arguments, by events -- the image is valid,
so every thread of the trace call reads its column and returns.  With --track T: frames_to_samples with links="unique" and with
links="trace" alternating, the pairs each emits, and what the frames that are still invalid fail by.
    python tools/vectorize_cost.py --trace [--rounds 50]
    python tools/vectorize_cost.py --track 64 --trace [--rounds 20]
--pinch neck adds the arms that read pinch windows as necks (pinch="neck", the _pinch_traj entry points).  On the 4 096 x 4 096
image, read as a one-image union: ggnn_image_junctions_traj and ggnn_image_junctions_pinch_traj(GGNN_PINCH_NECK) on prepared
arguments, by events, alternating with the other arms, and the image's n_pinch_windows.  With --track T: frames_to_samples with
pinch="junction" and with pinch="neck" alternating, and the pairs each emits.
--against LIB adds one arm to the plain run: ggnn_image_junctions of another build of the library (the parent commit's, say) on
the same prepared arguments, alternating with this build's within every round.
    python tools/vectorize_cost.py --pinch neck [--against /path/to/libggnn.so] [--rounds 20]
    python tools/vectorize_cost.py --track 64 --pinch neck [--rounds 20]
--label times the stage before all of these, segmenting a measured map (vectorize.label_grains, ggnn_label_grains), in angles mode
with K = 2 on two maps: frame 0 of tests/golden/pf_frames_cfg1.npz (501 x 501, 118 grains, as it is) and a --size x --size periodic
Voronoi map of size^2 / 8192 cells with 1 % of the pixels non-indexed or wrong (half each) and min_pixels = 8; and prints
  call       ggnn_label_grains on prepared arguments, by events
  label      one label_grains with its read-back, by the host clock
  host       the only route before it, by the host clock: the map read back, the links in numpy, scipy's connected components of
             the link graph (which takes the wrap and the tolerance as they are; scipy.ndimage.label takes one id a call, and the
             wrong pixels spread every id's bounding box over the whole map), the restatement's numbering and cleanup sweeps
             (tests/labelcheck.py), the image uploaded.  --host-rounds bounds its rounds (it takes seconds on the large map).
The arms alternate within a round; median of the rounds after three warm-up rounds.  Then the device activities of one call
for both maps (they must not differ: the launches do not depend on the content), the traffic floor of every launch (the bytes
it must move / 8 TB/s), and, where the tracer is there, the device time of every kernel.
    python tools/vectorize_cost.py --label [--rounds 20] [--size 4096] [--host-rounds 2] [--no-host]
--link times giving the grains of a labelled sequence ids that persist (vectorize.link_labels / label_sequence, ggnn_link_labels),
in ids mode on two sequences: the seven recorded frames of tests/golden/pf_frames_cfg1.npz (501 x 501, 118 grains falling to
100) and --track's drift sequence of 64 frames of --size x --size (128 when not given) with 121 grains; and prints
  call       ggnn_link_labels on prepared arguments (the stack labelled frame by frame on the device before), by events
  link       one link_labels on that stack with its read-back, by the host clock
  host       the only route before it, by the host clock: the labelled stack read back, the votes as one numpy bincount a pair
             of frames and the matcher of the restatement (tests/linkcheck.py), the relabelled stack uploaded
  sequence   one label_sequence, the labelling of every frame included, by the host clock
The arms alternate within a round; median of the rounds after three warm-up rounds.  Then the device activities of one call
at T = 2 and at T (they must not differ).  --no-host leaves the host arm out (a profiler's run: per-launch times come from
rocprofv3 --kernel-trace --stats around this tool).
    python tools/vectorize_cost.py --link [--rounds 20] [--size 128] [--no-host]
--label-orient times segmenting a map of full orientations under cubic symmetry (vectorize.label_orientations,
ggnn_label_orientations) beside --label's angle call on --label's two maps, the two alternating within a round (label_orient_cost).
    python tools/vectorize_cost.py --label-orient [--rounds 20] [--size 4096]
--label-stack times labelling a STACK of maps in one call (vectorize.label_maps, ggnn_label_grains_stack) in ids mode on --link's
two sequences and, with --big B, on B copies of --label's 4 096 x 4 096 Voronoi map (min_pixels 8; there the work dominates, not
the launches); and prints
  stack      ggnn_label_grains_stack on prepared arguments, by events
  singles    T x ggnn_label_grains on prepared arguments, by events
  sequence   one label_sequence (the stacked labelling, the linking, the read-back), by the host clock
The arms alternate within a round; median (min - max) of the rounds after three warm-up rounds.  Then, in a pass of their
own, the device activities of one stacked call at T = 2 and at T, for ids and for orientations (they must not differ, and
must be 2 memsets + 9 + 2 max_sweeps and 12 + 2 max_sweeps kernels), and the device time of every kernel at T.
    python tools/vectorize_cost.py --label-stack [--rounds 20] [--size 128] [--big 8]"""
import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--size", type=int, default=None, help="image side (default: 4096, with --union 128)")
    ap.add_argument("--boundary", choices=("periodic", "noflux"), default="periodic")
    ap.add_argument("--union", type=int, default=0, metavar="B")
    ap.add_argument("--track", type=int, default=0, metavar="T")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--trace", action="store_true", help="the links=\"trace\" arms")
    ap.add_argument("--pinch", choices=("junction", "neck"), default="junction", help="neck: the pinch=\"neck\" arms")
    ap.add_argument("--against", metavar="LIB", help="another build of libggnn.so: its ggnn_image_junctions as one more arm")
    ap.add_argument("--label", action="store_true", help="the cost of label_grains")
    ap.add_argument("--link", action="store_true", help="the cost of link_labels and label_sequence")
    ap.add_argument("--label-orient", action="store_true", help="the cost of label_orientations beside label_grains")
    ap.add_argument("--label-stack", action="store_true", help="the cost of label_maps against T x label_grains and label_sequence")
    ap.add_argument("--big", type=int, default=0, metavar="B", help="--label-stack: also B copies of the 4 096 x 4 096 Voronoi map")
    ap.add_argument("--host-rounds", type=int, default=2, help="--label: timed rounds of the host route on the large map")
    ap.add_argument("--no-host", action="store_true", help="--label: leave the host route out (a profiler's run)")
    a = ap.parse_args()
    sys.path[:0] = [os.path.dirname(HERE)]
    if a.size is None:
        a.size = 128 if a.union or a.track or a.link or a.label_stack else 4096
    if a.label_stack:
        return label_stack_cost(a)
    if a.link:
        return link_cost(a)
    if a.label_orient:
        return label_orient_cost(a)
    if a.label:
        return label_cost(a)
    if a.track:
        return track_cost(a)
    if a.union:
        return union_cost(a)
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
        if a.against:
            other = ctypes.CDLL(a.against)
            other.ggnn_image_junctions.restype = ctypes.c_int
            other.ggnn_image_junctions.argtypes = lib.ggnn_image_junctions.argtypes
            arms["junctions, --against"] = lambda: _lib.check(other.ggnn_image_junctions(ctypes.byref(A), _lib.current_stream()), "against")
        if a.pinch == "neck":
            u = vz._vectorize_union(vz._stack(image[None]), [n_grain], "cells", 2, None, a.boundary, pinch="neck")
            res, _ = vz._graphs_of(u, u["status"].tolist(), False)
            print(f"# one-image union, pinch=\"neck\": status {res['status'][0]}, valid {vz.status_is_valid(res['status'][0], a.boundary)}",
                  flush=True)
            U, pinched = u["calls"][0], _lib.ptr(u["status"][u["pinch_words"]:])
            arms["junctions_traj"] = lambda: _lib.check(lib.ggnn_image_junctions_traj(ctypes.byref(U), _lib.current_stream()), "traj")
            arms["junctions_pinch_traj, neck"] = lambda: _lib.check(lib.ggnn_image_junctions_pinch_traj(
                ctypes.byref(U), _lib.GGNN_PINCH_NECK, pinched, _lib.current_stream()), "pinch_traj")
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
            print(f"{name:26s} us/call by events: median {np.median(t):8.1f}  min {t.min():8.1f}  max {t.max():8.1f}", flush=True)
        if a.trace:
            trace_call_cost(a, image, n_grain)
        print(f"# torch {torch.__version__}, {torch.cuda.get_device_name()}", flush=True)


def trace_call_cost(a, image, n_grain):
    """ggnn_junction_links_traj and ggnn_junction_links_trace_traj on the image as a one-image union, by events."""
    import numpy as np
    import torch
    from graingraphnn_amd import _lib
    from graingraphnn_amd import vectorize as vz
    lib = _lib.load()
    v = vz._vectorize_union(vz._stack(image[None]), [n_grain], "cells", 2, None, a.boundary, links="trace")
    res, _ = vz._graphs_of(v, v["status"].tolist(), False)
    print(f"# one-image union, links=\"trace\": status {res['status'][0]}, valid {vz.status_is_valid(res['status'][0], a.boundary)}",
          flush=True)
    L, T = v["calls"][1], v["trace_call"]
    arms = {"links_traj": lambda: _lib.check(lib.ggnn_junction_links_traj(ctypes.byref(L), _lib.current_stream()), "links_traj"),
            "trace_traj": lambda: _lib.check(lib.ggnn_junction_links_trace_traj(ctypes.byref(T), _lib.current_stream()), "trace_traj")}
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
        print(f"{name:10s} us/call by events: median {np.median(t):8.1f}  min {t.min():8.1f}  max {t.max():8.1f}", flush=True)
    print(f"# trace_traj / links_traj = {np.median(times['trace_traj']) / np.median(times['links_traj']):.2f}", flush=True)


def lattice_images(B, size, seed, device, cells=11):
    """[B, size, size] int32 periodic Voronoi images of cells x cells seeds on a jittered brick lattice (every other row
    shifted by half a cell): ids 1 .. cells^2, nearest seed under the torus metric."""
    import torch
    gen = torch.Generator(device="cpu").manual_seed(seed)
    iy, ix = torch.meshgrid(torch.arange(cells), torch.arange(cells), indexing="ij")
    sx = (ix + 0.5 * (iy % 2) + 0.25).reshape(-1) / cells
    sy = (iy + 0.25).reshape(-1) / cells
    jitter = (torch.rand(B, 2, cells * cells, generator=gen) - 0.5) * (0.3 / cells)
    px = ((torch.arange(size, dtype=torch.float32) + 0.5) / size).to(device)
    out = []
    for b in range(B):
        x, y = (sx + jitter[b, 0]).to(device), (sy + jitter[b, 1]).to(device)
        dx = (px[None, :, None] - x[None, None, :]).abs()
        dy = (px[:, None, None] - y[None, None, :]).abs()
        dx, dy = torch.minimum(dx, 1 - dx), torch.minimum(dy, 1 - dy)
        out.append((dx * dx + dy * dy).argmin(dim=2).to(torch.int32) + 1)
    return torch.stack(out)


def union_cost(a):
    import time
    import numpy as np
    import torch
    from graingraphnn_amd import _lib, synthetic
    from graingraphnn_amd import vectorize as vz
    from graingraphnn_amd.backend import default_backend
    from graingraphnn_amd.synthetic import EDGE_TYPES
    if a.boundary != "periodic":
        raise SystemExit("--union times periodic stacks")
    B, size = a.union, a.size
    dev = torch.device("cuda", 0)
    lib, be = _lib.load(), default_backend()
    with torch.no_grad():
        candidates = lattice_images(B + B // 2 + 8, size, a.seed, dev)
        n_grain = int(candidates.max())
        status = vz.graphs_from_images(candidates, [n_grain] * len(candidates), strict=False)["status"]
        valid = [i for i, s in enumerate(status) if vz.status_is_valid(s)]
        print(f"# {len(valid)} of {len(candidates)} candidate images are valid structures", flush=True)
        if len(valid) < B:
            raise SystemExit("too few valid images: try another --seed")
        images = candidates[valid[:B]].contiguous()
        n_grains = [n_grain] * B
        rs = np.random.RandomState(a.seed)
        theta_x = [rs.uniform(0, np.pi / 2, n_grain) for _ in range(B)]
        theta_z = [rs.uniform(0, np.pi / 2, n_grain) for _ in range(B)]
        G, R, span = 2.0, 0.4, 6

        def loop():
            parts = []
            for b in range(B):
                x, ei, ea = vz.sample_from_image(images[b], theta_x[b], theta_z[b], G, R, span=span)
                parts.append(tuple({k: v.cpu().numpy() for k, v in d.items()} for d in (x, ei, ea)))
            x, ei, ea, _ = synthetic.disjoint_union(parts)
            out = tuple({k: torch.from_numpy(v).to(dev) for k, v in d.items()} for d in (x, ei, ea))
            torch.cuda.synchronize()
            return out

        def union():
            out = vz.samples_from_images(images, theta_x, theta_z, G, R, span=span)
            torch.cuda.synchronize()
            return out

        X, EI, EA = loop()
        UX, UEI, UEA, off = union()
        same = all(torch.equal(X[k], UX[k]) for k in X) and all(torch.equal(EI[et], UEI[et]) and torch.equal(EA[et], UEA[et])
                                                                 for et in EDGE_TYPES)
        print(f"# {B} images {size} x {size}, {n_grain} grains each, {off['joint'][-1]} junctions; the union equals the loop's "
              f"disjoint union bit for bit: {same}", flush=True)
        singles = [vz._vectorize(images[b], n_grain, "cells", 2, None) for b in range(B)]
        whole = vz._vectorize_union(images, n_grains, "cells", 2, None)
        torch.cuda.synchronize()

        def calls_single():
            for b, v in enumerate(singles):
                A, L, _, _ = v["calls"]
                v["counts"].zero_()
                be.image_compare(images[b], None, n_grain, None, v["counts"])
                _lib.check(lib.ggnn_image_junctions(ctypes.byref(A), _lib.current_stream()), "junctions")
                _lib.check(lib.ggnn_junction_links(ctypes.byref(L), _lib.current_stream()), "links")

        def calls_union():
            A, L, _, _ = whole["calls"]
            _lib.check(lib.ggnn_image_junctions_traj(ctypes.byref(A), _lib.current_stream()), "junctions_traj")
            _lib.check(lib.ggnn_junction_links_traj(ctypes.byref(L), _lib.current_stream()), "links_traj")

        def by_events(call):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            call()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) * 1e3

        def by_clock(call):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            return (time.perf_counter() - t0) * 1e6

        arms = {"loop": lambda: by_clock(loop), "union": lambda: by_clock(union),
                f"calls x {B}": lambda: by_events(calls_single), "calls": lambda: by_events(calls_union)}
        times = {k: [] for k in arms}
        for rnd in range(a.rounds + 3):
            for name, arm in arms.items():
                t = arm()
                if rnd >= 3:
                    times[name].append(t)
        for name, t in times.items():
            t = np.array(t)
            print(f"{name:10s} us: median {np.median(t):10.1f}  min {t.min():10.1f}  max {t.max():10.1f}", flush=True)
        print(f"# loop / union = {np.median(times['loop']) / np.median(times['union']):.1f}, calls x {B} / calls = "
              f"{np.median(times['calls x %d' % B]) / np.median(times['calls']):.1f}", flush=True)
        try:
            from torch.profiler import ProfilerActivity, profile
            for name, call in (("loop", loop), ("union", union), (f"calls x {B}", calls_single), ("calls", calls_union)):
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    call()
                    torch.cuda.synchronize()
                n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
                print(f"{name:10s} device activities (kernels, memsets, copies) in one pass: {n}", flush=True)
                if name == "calls":
                    for k in sorted(prof.key_averages(), key=lambda k: k.key):
                        t = getattr(k, "device_time_total", None)
                        t = getattr(k, "cuda_time_total", 0.0) if t is None else t
                        if t:
                            print(f"    {k.count:3d} x {k.key[:110]}: {t:.1f} us by the tracer", flush=True)
        except Exception as exc:   # (a build of torch without the tracer)
            print(f"# launches not counted: {type(exc).__name__}: {exc}", flush=True)
        print(f"# torch {torch.__version__}, {torch.cuda.get_device_name()}", flush=True)


def lattice_frames(T, size, seed, device, cells=11):
    """[T, size, size] int32: `lattice_images`' Voronoi image of one set of seeds that drift by a fraction of a pixel a frame."""
    import torch
    gen = torch.Generator(device="cpu").manual_seed(seed)
    iy, ix = torch.meshgrid(torch.arange(cells), torch.arange(cells), indexing="ij")
    sx = (ix + 0.5 * (iy % 2) + 0.25).reshape(-1) / cells + (torch.rand(cells * cells, generator=gen) - 0.5) * (0.3 / cells)
    sy = (iy + 0.25).reshape(-1) / cells + (torch.rand(cells * cells, generator=gen) - 0.5) * (0.3 / cells)
    vx, vy = ((torch.rand(2, cells * cells, generator=gen) - 0.5) * (0.6 / size))
    px = ((torch.arange(size, dtype=torch.float32) + 0.5) / size).to(device)
    out = []
    for t in range(T):
        x, y = (sx + t * vx).to(device), (sy + t * vy).to(device)
        dx = (px[None, :, None] - x[None, None, :]).abs()
        dy = (px[:, None, None] - y[None, None, :]).abs()
        dx, dy = torch.minimum(dx, 1 - dx), torch.minimum(dy, 1 - dy)
        out.append((dx * dx + dy * dy).argmin(dim=2).to(torch.int32) + 1)
    return torch.stack(out)


def track_cost(a):
    import time
    import numpy as np
    import torch
    sys.path[:0] = [os.path.join(os.path.dirname(HERE), "tests")]
    import trackcheck as tc
    from graingraphnn_amd import _lib
    from graingraphnn_amd import vectorize as vz
    from graingraphnn_amd.synthetic import EDGE_TYPES
    if a.boundary != "periodic":
        raise SystemExit("--track times periodic sequences")
    T, size = a.track, a.size
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    with torch.no_grad():
        frames = lattice_frames(T, size, a.seed, dev)
        n_grain = int(frames.max())
        rs = np.random.RandomState(a.seed)
        theta_x, theta_z = rs.uniform(0, np.pi / 2, n_grain), rs.uniform(0, np.pi / 2, n_grain)
        G, R, span = 2.0, 0.4, 6

        def host(frames=frames):
            res = vz.graphs_from_images(frames, [n_grain] * len(frames), strict=False)
            counts = torch.stack([torch.bincount(f.reshape(-1).long(), minlength=n_grain + 1)[1:] for f in frames]).reshape(-1)
            u = {"xy": res["xy"].cpu().numpy(), "triples": res["triples"].cpu().numpy(),
                 "jj": res["edge_index_dict"][EDGE_TYPES[2]].cpu().numpy(), "counts": counts.cpu().numpy(), "status": res["status"],
                 "joint_off": res["traj_offsets"]["joint"]}
            return tc.track(u, n_grain, "periodic", shape=(size, size))

        def samples(frames=frames, links="unique", pinch="junction"):
            out = vz.frames_to_samples(frames, theta_x, theta_z, G, R, span=span, links=links, pinch=pinch)
            torch.cuda.synchronize()
            return out

        r = host()
        got, report = samples()
        same = report["pairs"] == r["pairs"] and report["counts"] == [r["counts"][t] for t, _ in r["pairs"]] and all(
            np.array_equal(s[3]["joint"].cpu().numpy(), tc.cut(r, n_grain, t)[0]["joint"])
            and np.array_equal(s[3]["edge_event"].cpu().numpy(), tc.cut(r, n_grain, t)[0]["edge_event"])
            for (t, _), s in zip(r["pairs"], got))
        total = {k: sum(c[k] for c in report["counts"]) for k in vz.PAIR_COUNTERS}
        print(f"# {T} frames {size} x {size}, {n_grain} grains, {sum(s['n_joint'] for s in report['status'])} junctions, "
              f"{len(report['pairs'])} pairs emitted, {len(report['skipped'])} skipped; totals {total}; the samples equal the host "
              f"route's: {same}", flush=True)
        whole = {n: vz._track(frames[:n], n_grain, "cells", 2, None, "periodic") for n in sorted({min(8, T), T})}
        torch.cuda.synchronize()

        def calls(n=T):
            K, A = whole[n]["track_calls"][:2]
            _lib.check(lib.ggnn_track_junctions(ctypes.byref(K), _lib.current_stream()), "track_junctions")
            _lib.check(lib.ggnn_track_targets(ctypes.byref(A), _lib.current_stream()), "track_targets")

        def by_events(call):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            call()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) * 1e3

        def by_clock(call):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            return (time.perf_counter() - t0) * 1e6

        arms = {"host": lambda: by_clock(host), "samples": lambda: by_clock(samples), "calls": lambda: by_events(calls)}
        if a.trace:
            _, traced = samples(links="trace")
            still = [s for s in traced["status"] if not vz.status_is_valid(s)]
            euler = sum(1 for s in still if s["n_joint"] != 2 * s["n_present_grains"])
            print(f"# links=\"trace\": {len(traced['pairs'])} pairs emitted, {len(traced['skipped'])} skipped (links=\"unique\": "
                  f"{len(report['pairs'])} and {len(report['skipped'])}); {sum(s['n_traced'] for s in traced['status'])} columns traced "
                  f"in {sum(1 for s in traced['status'] if s['n_traced'])} frames; {len(still)} frames still invalid, {euler} of them "
                  f"by Euler's formula, with {sum(s['n_trace_failed'] for s in still)} failed and "
                  f"{sum(s['n_trace_overflow'] for s in still)} overflowed columns", flush=True)
            arms["samples, trace"] = lambda: by_clock(lambda: samples(links="trace"))
        if a.pinch == "neck":
            _, necked = samples(pinch="neck")
            still = [t for t, s in enumerate(necked["status"]) if not vz.status_is_valid(s)]
            print(f"# pinch=\"neck\": {len(necked['pairs'])} pairs emitted, {len(necked['skipped'])} skipped (pinch=\"junction\": "
                  f"{len(report['pairs'])} and {len(report['skipped'])}); {sum(necked['n_pinch_windows'])} pinch windows in "
                  f"{sum(1 for p in necked['n_pinch_windows'] if p)} frames; {sum(s['n_joint'] for s in necked['status'])} junctions; "
                  f"frames still invalid: {still}; totals "
                  f"{ {k: sum(c[k] for c in necked['counts']) for k in vz.PAIR_COUNTERS} }", flush=True)
            arms["samples, neck"] = lambda: by_clock(lambda: samples(pinch="neck"))
        times = {k: [] for k in arms}
        for rnd in range(a.rounds + 3):
            for name, arm in arms.items():
                t = arm()
                if rnd >= 3:
                    times[name].append(t)
        for name, t in times.items():
            t = np.array(t)
            print(f"{name:14s} us: median {np.median(t):10.1f}  min {t.min():10.1f}  max {t.max():10.1f}", flush=True)
        print(f"# host / samples = {np.median(times['host']) / np.median(times['samples']):.1f}", flush=True)
        try:
            from torch.profiler import ProfilerActivity, profile
            for n in sorted(whole):
                for name, call in (("vectorise + track", lambda: vz._track(frames[:n], n_grain, "cells", 2, None, "periodic")),
                                   ("calls", lambda: calls(n))):
                    with profile(activities=[ProfilerActivity.CUDA]) as prof:
                        call()
                        torch.cuda.synchronize()
                    k = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
                    print(f"T = {n:3d}  {name:18s} device activities (kernels, memsets, copies) in one pass: {k}", flush=True)
                    if name == "calls" and n == T:
                        for e in sorted(prof.key_averages(), key=lambda e: e.key):
                            t = getattr(e, "device_time_total", None)
                            t = getattr(e, "cuda_time_total", 0.0) if t is None else t
                            if t:
                                print(f"    {e.count:3d} x {e.key[:110]}: {t:.1f} us by the tracer", flush=True)
        except Exception as exc:   # (a build of torch without the tracer)
            print(f"# launches not counted: {type(exc).__name__}: {exc}", flush=True)
        print(f"# torch {torch.__version__}, {torch.cuda.get_device_name()}", flush=True)


def link_cost(a):
    import time
    import numpy as np
    import torch
    sys.path[:0] = [os.path.join(os.path.dirname(HERE), "tests")]
    import linkcheck as lk
    from graingraphnn_amd import _lib
    from graingraphnn_amd import vectorize as vz
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    d = np.load(os.path.join(os.path.dirname(HERE), "tests", "golden", "pf_frames_cfg1.npz"))
    sequences = {"recorded, 7 frames 501 x 501": torch.from_numpy(d["frames"].astype(np.int32)).to(dev),
                 f"drift, 64 frames {a.size} x {a.size}": lattice_frames(64, a.size, a.seed, dev)}

    def by_events(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3

    def by_clock(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    for name, ids in sequences.items():
        T, ny, nx = ids.shape
        cap = 256                                                   # room per frame: both sequences hold fewer than 128 grains
        per_frame = [vz._label(ids[t], None, None, None, 1, 64, "periodic", cap) for t in range(T)]
        labels = torch.stack([v["image"] for v in per_frame])
        n_local = torch.stack([v["status"] for v in per_frame])[:, 4].contiguous()

        def host_route():
            r = lk.link(labels.cpu().numpy(), n_local.tolist(), local_capacity=cap)
            out = torch.from_numpy(r["frames"]).to(dev)
            torch.cuda.synchronize()
            return out, r

        frames, n_grain, _, report = vz.link_labels(labels, n_local, local_capacity=cap)
        whole = {n: vz._link_checked(labels[:n].contiguous(), n_local[:n].contiguous(), None, None, 1, "periodic", cap, None) for n in sorted({2, T})}
        torch.cuda.synchronize()
        A = whole[T]["calls"][0]
        total = {k: sum(s[k] for s in report["frames"]) for k in vz.LINK_FRAME_WORDS[1:]}
        print(f"# {name}: {report['frames'][0]['n_local']} grains falling to {report['frames'][-1]['n_local']}, {n_grain} global; totals "
              f"{total}; workspace {lib.ggnn_link_workspace_bytes(T, cap, 0) / 1e6:.2f} MB", flush=True)
        if not a.no_host:
            h_frames, r = host_route()
            print(f"# the host route gives the same frames: {bool(torch.equal(h_frames, frames))}; status equal: "
                  f"{r['status'] == report['frames']}", flush=True)
        arms = {"call": lambda: by_events(lambda: _lib.check(lib.ggnn_link_labels(ctypes.byref(A), _lib.current_stream()), "link")),
                "link": lambda: by_clock(lambda: vz.link_labels(labels, n_local, local_capacity=cap)),
                "host": lambda: by_clock(host_route),
                "sequence": lambda: by_clock(lambda: vz.label_sequence(ids=ids, grain_capacity=cap))}
        if a.no_host:
            del arms["host"]
        times = {k: [] for k in arms}
        for rnd in range(a.rounds + 3):
            for arm, call in arms.items():
                t = call()
                if rnd >= 3:
                    times[arm].append(t)
        for arm, t in times.items():
            t = np.array(t)
            print(f"{arm:8s} us ({len(t)} rounds): median {np.median(t):12.1f}  min {t.min():12.1f}  max {t.max():12.1f}", flush=True)
        if not a.no_host:
            print(f"# host / link = {np.median(times['host']) / np.median(times['link']):.1f}", flush=True)
        try:
            from torch.profiler import ProfilerActivity, profile
            for n in sorted(whole):
                An = whole[n]["calls"][0]
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    _lib.check(lib.ggnn_link_labels(ctypes.byref(An), _lib.current_stream()), "link")
                    torch.cuda.synchronize()
                k = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
                print(f"T = {n:3d}  device activities (kernels, memsets) of one call: {k}", flush=True)
                if n == T:
                    for e in sorted(prof.key_averages(), key=lambda e: e.key):
                        t = getattr(e, "device_time_total", None)
                        t = getattr(e, "cuda_time_total", 0.0) if t is None else t
                        if t:
                            print(f"    {e.count:3d} x {e.key[:110]}: {t:.1f} us by the tracer", flush=True)
        except Exception as exc:   # (a build of torch without the tracer)
            print(f"# launches not counted: {type(exc).__name__}: {exc}", flush=True)
    print(f"# torch {torch.__version__}, {torch.cuda.get_device_name()}", flush=True)


def label_stack_cost(a):
    import time
    import numpy as np
    import torch
    from graingraphnn_amd import _lib
    from graingraphnn_amd import vectorize as vz
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    d = np.load(os.path.join(os.path.dirname(HERE), "tests", "golden", "pf_frames_cfg1.npz"))
    sequences = {"recorded, 7 frames 501 x 501": (torch.from_numpy(d["frames"].astype(np.int32)).to(dev), 1, 256, a.rounds),
                 f"drift, 64 frames {a.size} x {a.size}": (lattice_frames(64, a.size, a.seed, dev), 1, 256, a.rounds)}
    if a.big:
        big = argparse.Namespace(size=4096, seed=a.seed)
        ids = torch.from_numpy(measured_maps(big, dev)[2].astype(np.int32)).to(dev)
        sequences[f"Voronoi with 1 % noise, {a.big} frames 4096 x 4096"] = (ids[None].repeat(a.big, 1, 1), 8, 4096 * 4096 // 8 + 2,
                                                                           max(3, a.rounds // 4))

    def by_events(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3

    def by_clock(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def activities(call):
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA), prof

    for name, (ids, mp, cap, rounds) in sequences.items():
        T, ny, nx = ids.shape
        stacked = vz._label_stack(ids, None, None, None, mp, 64, "periodic", cap)
        singles = [vz._label(ids[t], None, None, None, mp, 64, "periodic", cap) for t in range(T)]
        torch.cuda.synchronize()
        same = all(torch.equal(stacked["image"][t], v["image"]) and torch.equal(stacked["status"][t], v["status"]) for t, v in enumerate(singles))
        grains = stacked["status"][:, 4].tolist()
        print(f"# {name}: grains per frame {grains[0]} .. {grains[-1]}, sweeps {stacked['status'][:, 5].tolist()}; the stacked call equals the "
              f"{T} single calls: {same}; workspace {lib.ggnn_label_stack_workspace_bytes(T, nx, ny, 0) / 1e6:.1f} MB against "
              f"{lib.ggnn_label_workspace_bytes(nx, ny, 0) / 1e6:.1f} MB a frame", flush=True)
        A, As = stacked["calls"][0], [v["calls"][0] for v in singles]

        def all_singles():
            for At in As:
                _lib.check(lib.ggnn_label_grains(ctypes.byref(At), _lib.current_stream()), "label")
        arms = {"stack": lambda: by_events(lambda: _lib.check(lib.ggnn_label_grains_stack(ctypes.byref(A), _lib.current_stream()), "stack")),
                "singles": lambda: by_events(all_singles)}
        if cap <= vz.LINK_MAX_DEFAULT_CAPACITY:                       # (the linking takes at most 65 536 rows a frame)
            arms["sequence"] = lambda: by_clock(lambda: vz.label_sequence(ids=ids, min_pixels=mp, grain_capacity=cap))
        times = {k: [] for k in arms}
        for rnd in range(rounds + 3):
            for arm, call in arms.items():
                t = call()
                if rnd >= 3:
                    times[arm].append(t)
        for arm, t in times.items():
            t = np.array(t)
            print(f"{arm:8s} us ({len(t)} rounds): median {np.median(t):12.1f}  ({t.min():.1f} - {t.max():.1f})", flush=True)
        print(f"# singles / stack = {np.median(times['singles']) / np.median(times['stack']):.2f}", flush=True)
        try:
            table = torch.randn(4, int(ids.max()) + 1, device=dev)
            table = (table / table.norm(dim=0)).to(torch.float32)
            for n in sorted({2, T}):
                few = ids[:n].contiguous()
                An = vz._label_stack(few, None, None, None, mp, 64, "periodic", cap)["calls"]
                k, prof = activities(lambda: _lib.check(lib.ggnn_label_grains_stack(ctypes.byref(An[0]), _lib.current_stream()), "stack"))
                quats = table[:, few.long()].permute(1, 0, 2, 3).contiguous()
                On = vz._label_orient_stack(quats, float(np.deg2rad(2.0)), None, mp, 64, "periodic", cap, "cubic")["calls"]
                ko, _ = activities(lambda: _lib.check(lib.ggnn_label_orientations_stack(ctypes.byref(On[0]), _lib.current_stream()), "stack"))
                print(f"T = {n:3d}  device activities (kernels, memsets) of one stacked call: ids {k} (2 + 9 + 2 x 64 = 139), orientations {ko} "
                      f"(2 + 12 + 2 x 64 = 142)", flush=True)
                del quats, On
                if n == T:
                    for e in sorted(prof.key_averages(), key=lambda e: e.key):
                        t = getattr(e, "device_time_total", None)
                        t = getattr(e, "cuda_time_total", 0.0) if t is None else t
                        if t:
                            print(f"    {e.count:3d} x {e.key[:110]}: {t:.1f} us by the tracer", flush=True)
        except Exception as exc:   # (a build of torch without the tracer)
            print(f"# launches not counted: {type(exc).__name__}: {exc}", flush=True)
        del stacked, singles
    print(f"# torch {torch.__version__}, {torch.cuda.get_device_name()}", flush=True)


def label_floor(nx, ny, K, status, max_sweeps):
    """[(launch, bytes it must move)] of one ggnn_label_grains: every array a pass reads or writes once, gathers of neighbours
    and roots counted as hits; the sweeps move the open pixels' words only."""
    N, n_open = nx * ny, status["n_invalid_in"] + status["n_speck_pixels"]
    seams = ny * -(-nx // 64) + nx * -(-ny // 16)
    out = [("links", N * (4 * K + 1)), ("tiles", N * (1 + 4 * K + 4)), ("seams", seams * 9), ("flatten", N * (1 + 4 + 4)),
           ("classify", N * (1 + 4 + 4) + 4 * n_open)]
    out += [(f"sweep {s}", n_open * (4 + 4 + 4) + n_open * (4 + 4 + 4)) for s in range(min(status["n_sweeps"] + 1, max_sweeps))]
    out += [("rank sums", 4 * N), ("rank scan", 8 * -(-N // 1024)), ("rank add", 4 * N), ("image", N * (4 + 4))]
    return out


def measured_maps(a, dev):
    """The two maps of --label and --label-orient -> (frame 0 of the recorded run as ids from 1, its (theta_x, theta_z) per grain,
    the ids of the noisy Voronoi map with 0 = non-indexed, its (theta_x, theta_z) per cell, its cells, the random state)."""
    import numpy as np
    import torch
    d = np.load(os.path.join(os.path.dirname(HERE), "tests", "golden", "pf_frames_cfg1.npz"))
    frame = d["frames"][0].astype(np.int64)
    theta = np.stack([d["theta_x"], d["theta_z"]]).astype(np.float32)
    rs = np.random.RandomState(a.seed)
    n = max(4, a.size * a.size // 8192)
    seeds = torch.from_numpy(rs.uniform(0, a.size, (n, 2)).astype(np.float32)).to(dev)   # nearest seed on the torus, in slabs of rows
    px = torch.arange(a.size, dtype=torch.float32, device=dev) + 0.5
    slabs = []
    for y0 in range(0, a.size, 16):
        dy = (px[y0:y0 + 16, None] - seeds[None, :, 0]).abs()
        dx = (px[:, None] - seeds[None, :, 1]).abs()
        dy, dx = torch.minimum(dy, a.size - dy), torch.minimum(dx, a.size - dx)
        slabs.append((dy[:, None, :] ** 2 + dx[None, :, :] ** 2).argmin(2))
    ids = torch.cat(slabs).cpu().numpy() + 1
    del slabs
    th = np.stack([np.linspace(0.05, 1.5, n)[rs.permutation(n)], np.linspace(1.5, 0.05, n)[rs.permutation(n)]]).astype(np.float32)
    m = rs.rand(a.size, a.size)
    ids[m < 0.005] = 0
    wrong = (m >= 0.005) & (m < 0.01)
    ids[wrong] = rs.randint(1, n + 1, int(wrong.sum()))
    return frame, theta, ids, th, n, rs


def label_orient_cost(a):
    """--label-orient: ggnn_label_orientations against ggnn_label_grains (angles, K = 2) on the two maps of --label, the
    orientations by the recipe of tests/orientcheck.py (an orientation a cell more than 5 degrees from every other; per pixel at
    most 0.3 degrees of noise, a random one of the 24 equivalents and a random sign; tol = 2 degrees).  The two calls alternate
    within a round, by events; median, min and max of the rounds after three warm-up rounds; then the device activities of one
    call, the tracer's time of every kernel and the traffic floors of the two added passes (links: four planes read, a byte
    written, 17 bytes a pixel; accumulate: the label and four planes of a closed pixel, 20 bytes, gathers of the root counted
    as hits, plus 32 bytes of atomics a run).  Per-launch times: rocprofv3 --kernel-trace --stats around this tool."""
    import numpy as np
    import torch
    sys.path[:0] = [os.path.join(os.path.dirname(HERE), "tests")]
    import orientcheck as oc
    from graingraphnn_amd import _lib
    from graingraphnn_amd import vectorize as vz
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    frame, theta, ids, th, n, rs = measured_maps(a, dev)
    tol = float(np.deg2rad(2.0))

    def cell_quats(count):
        q = oc.random_quats(rs, count)
        for i in range(1, count):
            while oc.disorientation(q[:, :i], np.repeat(q[:, i:i + 1], i, 1)).min() <= np.deg2rad(5.0):
                q[:, i] = oc.random_quats(rs, 1)[:, 0]
        return q

    def qmul(p, q):
        return torch.stack([p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3], p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
                            p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1], p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0]])

    def orientations(cells, cq):
        """cells [ny, nx] (ids from 1, 0 = non-indexed) -> float32 [4, ny, nx] on the device, by the recipe, in float64 there."""
        g = torch.Generator(device=dev).manual_seed(a.seed)
        flat = torch.from_numpy(cells.reshape(-1)).to(dev)
        N = flat.numel()
        axis = torch.randn(3, N, dtype=torch.float64, device=dev, generator=g)
        half = torch.rand(N, dtype=torch.float64, device=dev, generator=g) * (np.deg2rad(0.3) / 2)
        noise = torch.cat([torch.cos(half)[None], axis / axis.norm(dim=0) * torch.sin(half)])
        ops = torch.from_numpy(oc.ops64()).to(dev)[torch.randint(0, 24, (N,), device=dev, generator=g)].T
        sign = torch.randint(0, 2, (N,), device=dev, generator=g).to(torch.float64) * 2 - 1
        q = qmul(qmul(torch.from_numpy(cq).to(dev)[:, flat.clamp(min=1) - 1], noise), ops) * sign
        q[:, flat == 0] = float("nan")
        return q.to(torch.float32).reshape(4, *cells.shape).contiguous()

    maps = {"golden 501 x 501": (orientations(frame, cell_quats(theta.shape[1])), torch.from_numpy(np.ascontiguousarray(theta[:, frame - 1])).to(dev),
                                 1e-3, 1),
            f"voronoi {a.size} x {a.size}, {n} cells, 1 % noise": (orientations(ids, cell_quats(n)), None, 0.5 * 1.45 / n, 8)}
    big = torch.from_numpy(np.ascontiguousarray(th[:, np.maximum(ids, 1) - 1])).to(dev)
    big[:, torch.from_numpy(ids == 0).to(dev)] = float("nan")
    key = list(maps)[1]
    maps[key] = (maps[key][0], big) + maps[key][2:]

    def by_events(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3

    for name, (quats, angles, angle_tol, mp) in maps.items():
        _, ny, nx = quats.shape
        image, n_grain, means, status = vz.label_orientations(quats, tol, min_pixels=mp)
        a_image, a_n, _, a_status = vz.label_grains(angles=angles, tol=angle_tol, min_pixels=mp)
        print(f"# {name}: orientations {n_grain} grains, status {status}; angles {a_n} grains; the same image: "
              f"{bool(torch.equal(image, a_image))}; workspace {lib.ggnn_label_orient_workspace_bytes(nx, ny) / 1e6:.1f} MB", flush=True)
        O = vz._label_orient(quats, tol, None, mp, 64, "periodic", None, "cubic")["calls"][0]
        A = vz._label(None, angles, angle_tol, None, mp, 64, "periodic", None)["calls"][0]
        arms = {"orient": lambda: _lib.check(lib.ggnn_label_orientations(ctypes.byref(O), _lib.current_stream()), "orient"),
                "angles": lambda: _lib.check(lib.ggnn_label_grains(ctypes.byref(A), _lib.current_stream()), "label")}
        times = {k: [] for k in arms}
        for rnd in range(a.rounds + 3):
            for arm, call in arms.items():
                t = by_events(call)
                if rnd >= 3:
                    times[arm].append(t)
        for arm, t in times.items():
            t = np.array(t)
            print(f"{arm:6s} us ({len(t)} rounds): median {np.median(t):12.1f}  min {t.min():12.1f}  max {t.max():12.1f}", flush=True)
        N, closed = nx * ny, nx * ny - status["n_invalid_in"] - status["n_speck_pixels"]
        print(f"# traffic floors at 8 TB/s: orientation links {17 * N / 8e6:.2f} us ({17 * N / 1e6:.1f} MB), angle links (K = 2) "
              f"{9 * N / 8e6:.2f} us, accumulate {(4 * N + 16 * closed) / 8e6:.2f} us ({closed} closed pixels) plus the atomics, "
              f"zero {4 * N / 8e6:.2f} us, means {4 * N / 8e6:.2f} us", flush=True)
        try:
            from torch.profiler import ProfilerActivity, profile
            for arm, call in arms.items():
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    call()
                    torch.cuda.synchronize()
                count = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
                print(f"{arm}: device activities (kernels, memsets) of one call: {count}", flush=True)
                for e in sorted(prof.key_averages(), key=lambda e: e.key):
                    t = getattr(e, "device_time_total", None)
                    t = getattr(e, "cuda_time_total", 0.0) if t is None else t
                    if t:
                        print(f"    {e.count:3d} x {e.key[:100]}: {t:.1f} us by the tracer", flush=True)
        except Exception as exc:   # (a build of torch without the tracer)
            print(f"# launches not counted: {type(exc).__name__}: {exc}", flush=True)
    print(f"# torch {torch.__version__}, {torch.cuda.get_device_name()}", flush=True)


def label_cost(a):
    import time
    import numpy as np
    import torch
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    sys.path[:0] = [os.path.join(os.path.dirname(HERE), "tests")]
    import labelcheck as lc
    from graingraphnn_amd import _lib
    from graingraphnn_amd import vectorize as vz
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    frame, theta, ids, th, n, _ = measured_maps(a, dev)
    maps = {"golden 501 x 501": (np.ascontiguousarray(theta[:, frame - 1]), 1e-3, 1)}
    big = np.ascontiguousarray(th[:, np.maximum(ids, 1) - 1])
    big[:, ids == 0] = np.nan
    maps[f"voronoi {a.size} x {a.size}, {n} cells, 1 % noise"] = (big, 0.5 * 1.45 / n, 8)

    def host_route(angles_dev, tol, min_pixels):
        ang = angles_dev.cpu().numpy()
        ny, nx = ang.shape[1:]
        ok = lc.validity(None, ang, None)
        right, down = lc.links(None, ang, tol, ok, True)
        idx = np.arange(ny * nx, dtype=np.int64).reshape(ny, nx)
        src = np.concatenate([idx[right], idx[down]])
        dst = np.concatenate([np.roll(idx, -1, 1)[right], np.roll(idx, -1, 0)[down]])
        _, comp = connected_components(coo_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(ny * nx, ny * nx)), directed=False)
        first = np.full(comp.max() + 1, ny * nx, np.int64)
        np.minimum.at(first, comp, idx.reshape(-1))
        root = first[comp]
        okf = ok.reshape(-1)
        size = np.bincount(root[okf], minlength=ny * nx)
        closed = okf & (size[root] >= min_pixels)
        state = np.where(closed, root, -1).reshape(ny, nx)
        for _ in range(64):
            state, assigned = lc.sweep(state, True)
            if not assigned:
                break
        roots = np.unique(root[closed])
        rank = np.zeros(ny * nx + 1, np.int32)
        rank[roots] = np.arange(1, len(roots) + 1)
        image = torch.from_numpy(rank[state.reshape(-1)].reshape(ny, nx)).to(dev)
        torch.cuda.synchronize()
        return image, len(roots)

    def by_events(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3

    def by_clock(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    activities = {}
    for name, (angles, tol, mp) in maps.items():
        ang = torch.from_numpy(angles).to(dev)
        K, ny, nx = ang.shape
        image, n_grain, means, status = vz.label_grains(angles=ang, tol=tol, min_pixels=mp)
        v = vz._label(None, ang, tol, None, mp, 64, "periodic", None)
        A = v["calls"][0]
        print(f"# {name}: {n_grain} grains, status {status}, workspace {lib.ggnn_label_workspace_bytes(nx, ny, K) / 1e6:.1f} MB", flush=True)
        if not a.no_host:
            h_image, h_n = host_route(ang, tol, mp)
            print(f"# the host route gives the same image: {bool(torch.equal(h_image, image))} ({h_n} grains)", flush=True)
        large = nx * ny > 1 << 20
        arms = {"call": lambda: by_events(lambda: _lib.check(lib.ggnn_label_grains(ctypes.byref(A), _lib.current_stream()), "label")),
                "label": lambda: by_clock(lambda: vz.label_grains(angles=ang, tol=tol, min_pixels=mp)),
                "host": lambda: by_clock(lambda: host_route(ang, tol, mp))}
        if a.no_host:
            del arms["host"]
        times = {k: [] for k in arms}
        for rnd in range(a.rounds + 3):
            for arm, call in arms.items():
                if arm == "host" and large and not 3 <= rnd < 3 + a.host_rounds:
                    continue
                t = call()
                if rnd >= 3:
                    times[arm].append(t)
        for arm, t in times.items():
            t = np.array(t)
            print(f"{arm:6s} us ({len(t)} rounds): median {np.median(t):12.1f}  min {t.min():12.1f}  max {t.max():12.1f}", flush=True)
        if not a.no_host:
            print(f"# host / label = {np.median(times['host']) / np.median(times['label']):.1f}", flush=True)
        floor = label_floor(nx, ny, K, status, 64)
        total = sum(b for _, b in floor)
        print("# traffic floor at 8 TB/s: " + ", ".join(f"{k} {b / 8e6:.2f} us" for k, b in floor) + f"; all {total / 8e6:.1f} us "
              f"({total / 1e6:.1f} MB); call / floor = {np.median(times['call']) / (total / 8e6):.1f}", flush=True)
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                _lib.check(lib.ggnn_label_grains(ctypes.byref(A), _lib.current_stream()), "label")
                torch.cuda.synchronize()
            activities[name] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
            print(f"device activities (kernels, memsets) of one call: {activities[name]}", flush=True)
            for e in sorted(prof.key_averages(), key=lambda e: e.key):
                t = getattr(e, "device_time_total", None)
                t = getattr(e, "cuda_time_total", 0.0) if t is None else t
                if t:
                    print(f"    {e.count:3d} x {e.key[:100]}: {t:.1f} us by the tracer", flush=True)
        except Exception as exc:   # (a build of torch without the tracer)
            print(f"# launches not counted: {type(exc).__name__}: {exc}", flush=True)
    print(f"# device activities per map: {activities}; torch {torch.__version__}, {torch.cuda.get_device_name()}", flush=True)


if __name__ == "__main__":
    main()
