"""Start a rollout from a grain-ID image: the junction graph of a periodic or a no-flux image, found on the device.

`grain_image()` maps a layer's polygons to an image; this is the inverse.  A structure that exists as an image -- an EBSD
map, a phase-field cross-section with one grain id per pixel -- becomes the `(x_dict, edge_index_dict, edge_attr)` that
`GrainRollout` takes.  The reference has no such step (its graphs come from its generator or from its phase-field solver's
junction tracks, graph_trajectory.py:316-376).  The rule is include/ggnn.h's (ggnn_image_junctions, ggnn_junction_links),
restated in numpy by tests/vectorcheck.py: a junction is a 2 x 2 window of pixels with three distinct ids (four: two
junctions, split along the TL-BR diagonal), windows that repeat a triple within `merge_radius` are one junction at their
mean, junctions are numbered in raster order, and two junctions are linked when they share two grains.

On the phase-field frame 0 of the reference's seed 10020 (tests/golden/grain_image_cfg1.npz) this gives the reference's
own graph up to numbering: the same 236 triples, the same 354 junction pairs, every coordinate within half a pixel and
the area feature bit for bit.

`boundary="noflux"` takes an image with walls, non-square ones included: everything outside the image is grain 0, the
boundary grain of the reference's no-flux graphs (id 1, which does not occur inside), so a junction lies on a wall exactly
when its triple holds grain 0, wall junctions are linked along the walls through the pairs (0, a), their coordinate normal
to the wall is exactly 0, 1 or `max_y`, and the four corner pixels come back as the `corner_grains` that `grain_image`
fills the corners from (tests/vectorcheck_noflux.py restates the rule).

A STACK of equal-shaped images becomes one disjoint union in one go (`graphs_from_images`, `samples_from_images`;
ggnn_image_junctions_traj, ggnn_junction_links_traj; tests/vectorcheck_union.py): the rule per image, grains and
junctions numbered image after image, a status per image, and the trajectory offsets that `GrainRollout(traj_offsets=)`,
`enable_events`, `enable_qoi` and `enable_polygons` take.  The launches do not depend on the number of images and there is
one read-back.  The frames of a recorded sequence go the same way, each vectorised on its own.

A recorded SEQUENCE of images with stable grain ids becomes a training set (`frames_to_samples`, `track_frames`;
ggnn_track_junctions, ggnn_track_targets; tests/trackcheck.py): junctions of consecutive valid frames are matched
by their grain triple -- the reference's own mask rule, form_gradient:884-889 --, and the node targets, masks, grain events,
edge labels and history columns of `training.DeviceDataset`'s samples are derived from the match on the device, what the
reference gets from its junction tracker (graph_trajectory.py:283-846) and form_gradient (graph_datastruct.py:851-1011).

`links="trace"` adds a second linking rule to all of these (ggnn_image_junction_windows_traj, ggnn_junction_links_trace_traj;
tests/tracecheck.py): a pair of grains that more than one other junction holds -- two grains that share two separate
stretches of boundary: a lens on a boundary, a band from wall to wall -- is linked by following the boundary through the image,
on the device and exact in integers; the default `links="unique"` is the rule above, launch for launch.

`pinch="neck"` reads one window pattern differently in all of these (the _pinch_traj entry points; tests/pinchcheck.py; DESIGN
8s): three ids in a 2 x 2 window with the repeated one on a diagonal, [a b; c a], is grain a running through the pixel corner as
a neck, not a junction of a, b and c, and carries no key.  That is what an image looks like whose cell edges drift below a
pixel, and what the junction rule calls invalid by one junction too many; no pixel changes and no grain is renumbered.  The
default `pinch="junction"` is the rule above, launch for launch.

A MEASURED map is not a grain-ID image: it carries orientations per pixel, non-indexed points and speckle.  `label_grains`
(ggnn_label_grains; tests/labelcheck.py) is the stage before all of the above: connected components of an
orientation map (two neighbours are linked when every angle differs by at most `tol`) or of a noisy id image, periodic or with
walls, specks and non-indexed pixels dissolved into their neighbours by majority, grains numbered in raster order, and the
per-grain mean angles as exact fixed-point sums -- on the device, exact in integers.  `sample_from_orientations` chains it
with `sample_from_image`.  One wrong pixel on a boundary no longer drops a frame: it is repaired before the vectoriser,
whose own contract -- an invalid structure is reported, not repaired -- stands.

An EBSD map carries a full orientation per pixel, a Bunge triple that the indexing software reports as any of the 24 cubic
equivalents, changing from pixel to pixel inside one grain.  `label_orientations` (ggnn_label_orientations;
tests/orientcheck.py) is `label_grains` with the link decided by the disorientation of two neighbouring quaternions
under the cubic group, and a symmetry-aware mean orientation per grain; `quaternions_from_bunge` makes its input,
`growth_angles` turns a mean orientation into the model's theta_x and theta_z (the <100> direction nearest the sample's z),
`sample_from_euler_map` chains them with `sample_from_image`, and `label_orientation_sequence` /
`samples_from_euler_sequence` do for a series of such maps what `label_sequence` / `samples_from_orientation_sequence` do below.

Not covered: stacks of mixed image shapes, resolving a quadruple from a history (the diagonal is fixed, and counted in the
status), the reference's `edge` length target (its edge_len head is disabled in every shipped configuration) and its
`elim_list` scaling of shrinking grains (commented out in the reference); for the labelling: stacks of maps in one launch,
8-connectivity, hexagonal and other symmetry groups; for the linking: merging grains, a grain that reappears keeping its id,
matching across more than one frame back, crystal symmetry in the gate.

A SEQUENCE of measured maps gets ids that persist from frame to frame (`link_labels`, `label_sequence`,
`samples_from_orientation_sequence`; ggnn_link_labels; tests/linkcheck.py): every frame is labelled on its own, the
grains of consecutive frames are linked by their pixel overlap on the device -- votes in integers, the predecessor with the
most shared pixels, one keeper per predecessor, fresh ids for the rest --, and the relabelled stack is what `frames_to_samples`
takes: a series of measured maps becomes a training set without the host."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .backend import default_backend
from .synthetic import EDGE_TYPES

STATUS_WORDS = ("n_joint", "n_quad_windows", "n_merged_windows", "n_invalid_pixels", "n_open_pairs", "n_present_grains",
                "overflow")
GRIDS = {"cells": lambda nx: (np.float32(1.0), np.float32(1.0) / np.float32(nx)),
         "points": lambda nx: (np.float32(0.5), np.float32(1.0) / np.float32(nx - 1))}


BOUNDARIES = {"periodic": _lib.BC_PERIODIC, "noflux": _lib.BC_NOFLUX}
LINKS = ("unique", "trace")
TRACE_COUNTERS = ("n_traced", "n_trace_failed", "n_trace_overflow")
PINCHES = {"junction": _lib.GGNN_PINCH_JUNCTION, "neck": _lib.GGNN_PINCH_NECK}
EULER = {"periodic": "n_joint == 2 n_present_grains", "noflux": "n_joint == 2 n_present_grains - 2"}


def status_is_valid(status, boundary="periodic"):
    """Euler's formula -- on the torus two junctions a grain; on the sphere, with the boundary grain as the outer face of a
    no-flux image, two fewer -- and nothing dropped on the way."""
    _check_boundary(boundary)
    return (status["overflow"] == 0 and status["n_invalid_pixels"] == 0 and status["n_open_pairs"] == 0
            and status["n_joint"] == 2 * status["n_present_grains"] - (2 if boundary == "noflux" else 0))


def _check_boundary(boundary):
    if boundary not in BOUNDARIES:
        raise _lib.GGNNError(f"boundary must be 'periodic' or 'noflux', got {boundary!r}")


def _check_links(links, max_trace, nx, ny):
    """-> max_trace as the trace call takes it (None: 4 (nx + ny)), or None for links="unique"."""
    if links not in LINKS:
        raise ValueError(f"links must be 'unique' or 'trace', got {links!r}")
    if links == "unique":
        return None
    max_trace = 4 * (nx + ny) if max_trace is None else int(max_trace)
    if max_trace < 1:
        raise ValueError(f"max_trace must be at least 1, got {max_trace}")
    return max_trace


def _check_pinch(pinch):
    if pinch not in PINCHES:
        raise ValueError(f"pinch must be 'junction' or 'neck', got {pinch!r}")


def image_max_y(nx, ny, grid):
    """The far y wall of a no-flux [ny, nx] image, the kernel's own fp32 expression: ny / nx for "cells",
    (ny - 1) / (nx - 1) for "points", exactly 1 for a square image."""
    f = np.float32
    two_off = f(f(2) * GRIDS[grid](nx)[0])
    return float(f(f(f(ny - 2) + two_off) / f(f(nx - 2) + two_off)))


IMAGE_2D = "image must be a [ny, nx] device tensor of grain ids (pixel p = grain p - 1)"


def _image_tensor(t, dim, shape_text, noun="image"):
    """An image (dim 2) or a stack (dim 3) as the calls take it: on the device, integer -> int32, contiguous."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != dim:
        raise _lib.GGNNError(shape_text)
    if t.dtype not in (torch.int16, torch.int32, torch.int64, torch.uint8):
        raise _lib.GGNNError(f"{noun} must hold integers")
    return t.to(torch.int32).contiguous()


def _arrays(dev, n_grain, cap, n_image, ny, nx, noflux, status_words):
    """What both vectorisations write into, for `cap` junctions of `n_grain` grains in `n_image` [ny, nx] images:
    -> xy, triples, gj, jj, the zeroed status tensor of `status_words` words and the workspace."""
    xy = torch.zeros(cap, 2, dtype=torch.float32, device=dev)
    triples = torch.zeros(cap, 3, dtype=torch.int32, device=dev)
    # The joint->grain table is built for the capacity, before n_joint is known on the host.  The columns the kernel does
    # not write (junctions n_joint .. capacity) point spare grain rows of their own, n_grain + j, at junction j: the first
    # n_grain rows hold the real junctions alone, and no row grows long (the table's build sorts a row serially).
    slots = torch.arange(cap, dtype=torch.int64, device=dev).repeat_interleave(3)
    gj = torch.stack([slots + n_grain, slots])
    jj = torch.full((2, 3 * cap), -1, dtype=torch.int64, device=dev)
    status = torch.zeros(status_words, dtype=torch.int64, device=dev)
    wy, wx = (ny + 1, nx + 1) if noflux else (ny, nx)   # the rows of windows, the windows of a row
    words = n_image * wy * ((wx + _lib.GGNN_JUNCTION_SEGMENT - 1) // _lib.GGNN_JUNCTION_SEGMENT)
    ws = torch.empty(max(words, 1), dtype=torch.int32, device=dev)
    return xy, triples, gj, jj, status, ws


def _vectorize(image, n_grain, grid, merge_radius, joint_capacity, boundary="periodic"):
    """Every launch, no read-back: -> dict of the capacity-sized device arrays, the pixel counts, the joint->grain table
    and the status words (no-flux: the four corner pixels behind them, so that one read-back fetches both)."""
    be = default_backend()
    _check_boundary(boundary)
    noflux = boundary == "noflux"
    image = _image_tensor(image, 2, IMAGE_2D)
    if grid not in GRIDS:
        raise _lib.GGNNError(f"grid must be 'cells' or 'points', got {grid!r}")
    ny, nx = image.shape
    if n_grain is None:
        n_grain = int(image.max())   # (a read-back of its own: pass n_grain to avoid it)
    n_grain, R = int(n_grain), int(merge_radius)
    if n_grain < 1:
        raise _lib.GGNNError("n_grain must be at least 1")
    cap = 3 * n_grain + 16 if joint_capacity is None else int(joint_capacity)
    _, counts = be.image_compare(image, None, n_grain)
    W = _lib.GGNN_JUNCTION_STATUS_WORDS
    xy, triples, gj, jj, status, ws = _arrays(image.device, n_grain, cap, 1, ny, nx, noflux, W + (4 if noflux else 0))
    if noflux:   # the order of grain_image(corner_grains=)
        status[W:] = torch.stack([image[0, 0], image[0, -1], image[-1, 0], image[-1, -1]])
    off, pitch = GRIDS[grid](nx)
    A = _lib.JunctionArgs()
    A.image, A.pixel_counts, A.xy, A.triples = _lib.ptr(image), _lib.ptr(counts), _lib.ptr(xy), _lib.ptr(triples)
    A.edge_gj, A.status, A.workspace, A.workspace_bytes = _lib.ptr(gj), _lib.ptr(status), _lib.ptr(ws), 4 * ws.numel()
    A.nx, A.ny, A.n_grain, A.joint_capacity = nx, ny, n_grain, cap
    A.offset, A.pitch, A.merge_radius, A.boundary = float(off), float(pitch), R, BOUNDARIES[boundary]
    _lib.check(be.lib.ggnn_image_junctions(ctypes.byref(A), _lib.current_stream()), "ggnn_image_junctions")
    csr = be.build_csr_batch([(gj.flip(0).contiguous(), cap, n_grain + cap)], check=False)[0]
    L = _lib.LinkArgs()
    L.triples, L.rowptr, L.col, L.edge_jj, L.status = (_lib.ptr(triples), _lib.ptr(csr.rowptr), _lib.ptr(csr.col),
                                                       _lib.ptr(jj), _lib.ptr(status))
    L.n_grain, L.joint_capacity, L.E_cap = n_grain, cap, csr.col.numel()
    _lib.check(be.lib.ggnn_junction_links(ctypes.byref(L), _lib.current_stream()), "ggnn_junction_links")
    return {"xy": xy, "triples": triples, "gj": gj, "jj": jj, "status": status, "counts": counts, "csr": csr,
            "n_grain": n_grain, "capacity": cap, "shape": (ny, nx), "boundary": boundary,
            "max_y": image_max_y(nx, ny, grid) if noflux else None,
            "calls": (A, L, image, ws)}   # (the two calls' arguments and what they point to: tools/vectorize_cost.py)


def graph_from_image(image, n_grain=None, grid="cells", merge_radius=2, joint_capacity=None, strict=True,
                     boundary="periodic", links="unique", max_trace=None, pinch="junction"):
    """The junction graph of a grain-ID image, periodic or (boundary="noflux") with walls.

    image: integer [ny, nx] on the device, pixel p = grain p - 1 (what `grain_image` writes); n_grain: the number of grains
    (None: the image's largest id, at the price of a read-back); grid: "cells" -- pixel (y, x) covers
    [x / nx, (x + 1) / nx), the rasteriser's convention -- or "points" -- samples at x / (nx - 1), both ends included (the
    phase-field data's 501 points); merge_radius: windows that carry a triple within this Chebyshev distance of one another
    are one junction; joint_capacity: room for the junctions (default 3 n_grain + 16: a valid structure has 2 a grain).

    -> (xy float32 [n_joint, 2], triples int32 [n_joint, 3] of 0-based grains, edge_index_dict of int64 [2, 3 n_joint] for the
    three edge types, status dict).  Setup work: a dozen launches and ONE read-back, of the status.  strict: raise ValueError
    naming the counters unless the structure is valid (status_is_valid); strict=False returns it as it is, with -1 as the
    destination of every joint->joint column whose pair of grains has no partner, or more than one.

    boundary="noflux": the image is not periodic and may be non-square; everything outside it is grain 0, so the ids inside
    are 2 .. n_grain (n_grain counts the boundary grain; id 1 inside is an invalid pixel), a valid structure has
    2 n_present_grains - 2 junctions, and the junctions of grain 0 lie on the walls x = 0, x = 1, y = 0 and y = max_y.
    -> (xy, triples, edge_index_dict, status, corner_grains, max_y): the four as above, the ids of the corner pixels [0, 0],
    [0, nx - 1], [ny - 1, 0], [ny - 1, nx - 1] as `grain_image(corner_grains=)` takes them (they come with the status: still
    one read-back), and the far y wall as a float that is exact in fp32, for `GrainRollout(boundary="noflux", max_y=)`.

    links="unique" (the default) is the rule above: a pair of grains that MORE than one other junction holds stays open, and
    the structure is invalid -- which is what two grains look like that share two separate stretches of boundary: a lens on a
    boundary, a band from wall to wall.  links="trace" links those columns too, by following the boundary through the image
    from the junction to the one at its other end (ggnn_junction_links_trace_traj; tests/tracecheck.py), on the
    device and exact in integers; max_trace bounds a walk (None: 4 (nx + ny) vertices).  The image goes through the one-image
    union, which equals this path bit for bit; a structure without open pairs comes out as with "unique".  The status gains
    n_traced, n_trace_failed and n_trace_overflow (directed columns), n_open_pairs is what is still open, and strict judges
    that.  Still one read-back.  Any other value raises ValueError.

    pinch="junction" (the default) reads a PINCH WINDOW -- three distinct ids whose repeated id sits on a diagonal, [a b; c a] or
    [b a; a c] -- as the rule above does, as a junction of a, b and c.  It is none: grain a runs through the pixel corner as a
    neck, b and c do not meet, and the junction is one too many for Euler's formula, which is what an image with cell edges
    shorter than a pixel fails by.  pinch="neck" gives such a window no key (include/ggnn.h; tests/pinchcheck.py):
    no pixel changes and no grain is renumbered, the image goes through the one-image union as with links="trace", the status
    gains n_pinch_windows, and it combines with links="trace" and both boundaries.  A grain with a part that is not even
    corner-connected to its body stays invalid.  Any other value raises ValueError."""
    xy, triples, ei, status, v = _graph(image, n_grain, grid, merge_radius, joint_capacity, strict, boundary, links, max_trace,
                                        pinch)
    if boundary == "noflux":
        return xy, triples, ei, status, v["corner_grains"], v["max_y"]
    return xy, triples, ei, status


def _graph(image, n_grain, grid, merge_radius, joint_capacity, strict, boundary="periodic", links="unique", max_trace=None,
           pinch="junction"):
    """graph_from_image's four, with the capacity-sized arrays behind its results as a fifth."""
    _check_links(links, max_trace, 1, 1)
    _check_pinch(pinch)
    if links == "unique" and pinch == "junction":
        v = _vectorize(image, n_grain, grid, merge_radius, joint_capacity, boundary)
        words = v["status"].tolist()
        status = dict(zip(STATUS_WORDS, words))
        v["corner_grains"] = tuple(words[len(STATUS_WORDS):]) if boundary == "noflux" else None
        v["grain_counts"] = v["counts"][1:]   # (ggnn_image_compare's histogram is by id, from 0; a union's is by grain)
    else:   # the one-image union: the same bits, and the trace and pinch calls exist for unions alone
        _check_boundary(boundary)
        image = _image_tensor(image, 2, IMAGE_2D, "images")
        _check_links(links, max_trace, image.size(1), image.size(0))
        if n_grain is None:
            n_grain = int(image.max())   # (a read-back of its own: pass n_grain to avoid it)
        v = _vectorize_union(_stack(image[None]), [int(n_grain)], grid, merge_radius, joint_capacity, boundary, links=links,
                             max_trace=max_trace, pinch=pinch)
        res, _ = _graphs_of(v, v["status"].tolist(), False)   # the one read-back
        status = res["status"][0]
        v["corner_grains"] = res["corner_grains"][0] if boundary == "noflux" else None
        v["grain_counts"] = v["counts"]
    if strict and not status_is_valid(status, boundary):
        raise ValueError(f"the image is not a valid {boundary} grain structure: {status} (valid: overflow, n_invalid_pixels "
                         f"and n_open_pairs 0 and {EULER[boundary]}; joint_capacity {v['capacity']})")
    return (*_cut(v, min(status["n_joint"], v["capacity"])), status, v)


def _cut(v, n):
    """The first n junctions of the capacity-sized arrays: -> xy [n, 2], triples [n, 3], the three edge lists [2, 3 n]."""
    gj = v["gj"][:, :3 * n].contiguous()
    ei = {EDGE_TYPES[0]: gj, EDGE_TYPES[1]: gj.flip(0).contiguous(), EDGE_TYPES[2]: v["jj"][:, :3 * n].contiguous()}
    return v["xy"][:n].contiguous(), v["triples"][:n].contiguous(), ei


def sample_from_image(image, theta_x, theta_z, G, R, span=None, patch_pixels=None, **kw):
    """A rollout's first state from a grain-ID image: device (x_dict, edge_index_dict, edge_attr) in the layout and dtypes of
    `generator.reference_sample` (11 grain columns, 8 joint columns, global coordinates), as `GrainRollout` takes them.

    theta_x, theta_z: the grains' orientation angles [n_grain] (host; their cos / sin are formed in float64 and rounded
    once); G, R: the process parameters; span: the frame span (None: `synthetic.span_for(G, R)`); patch_pixels: the pixels
    of one training-size patch, the area feature being fp32(count / patch_pixels) of a double quotient (None: nx ny).
    Grain centres come from ggnn_grain_centres on the junctions found, edge lengths from the rollout's own edge refresh;
    the gradient columns are 0.  Other keywords go to `graph_from_image` (links="trace" among them: a grain with two sides, a
    lens, and the doubled joint->joint column between its two junctions are plain list entries; and pinch="neck": a raster with
    sub-pixel edges is read, not refused); an invalid structure always raises.

    boundary="noflux": the angles count the boundary grain, theta[0], and the result is what
    `GrainRollout(..., boundary="noflux", max_y=image_max_y(nx, ny, grid))` takes: the FULL edge lists, grain 0's edges
    included (the rollout masks them itself); grain 0's row as the reference keeps it -- centre (0.5, 0.5), area 0, extraV 0 --
    and every other centre from ggnn_grain_centres in its GGNN_BC_NOFLUX mode.  The rollout's boundary step finds this
    state as it would leave it."""
    from .synthetic import span_for
    theta_x, theta_z = np.asarray(theta_x, np.float64).ravel(), np.asarray(theta_z, np.float64).ravel()
    n_grain = int(kw.pop("n_grain", None) or len(theta_x))
    if len(theta_x) != n_grain or len(theta_z) != n_grain:
        raise _lib.GGNNError("theta_x and theta_z must hold one angle per grain")
    kw.pop("strict", None)
    boundary = kw.pop("boundary", "periodic")
    xy, _, ei, _, v = _graph(image, n_grain, kw.pop("grid", "cells"), kw.pop("merge_radius", 2),
                             kw.pop("joint_capacity", None), True, boundary, kw.pop("links", "unique"), kw.pop("max_trace", None),
                             kw.pop("pinch", "junction"))
    if kw:
        raise TypeError(f"sample_from_image: unknown keywords {sorted(kw)}")
    if span is None:
        span = span_for(G, R)
    # the union of one trajectory: its boundary grain is grain 0, and strict has judged it valid
    return _union_state(xy, ei, [0, xy.size(0)], v, v["grain_counts"], 0, True, [theta_x], [theta_z], [G], [R], span, patch_pixels)


# ---- a stack of images into one union ------------------------------------------------------------------------------------

def _stack(images):
    """[B, ny, nx] int32, contiguous, on the device, from a tensor or a list of equal-shaped [ny, nx] tensors."""
    if isinstance(images, (list, tuple)):
        if not images or any(not isinstance(i, torch.Tensor) or i.dim() != 2 or i.shape != images[0].shape for i in images):
            raise _lib.GGNNError("images must be equal-shaped [ny, nx] device tensors (one shape a stack)")
        images = torch.stack(list(images))
    shape_text = "images must be a [B, ny, nx] device tensor of grain ids, or a list of [ny, nx] device tensors"
    if isinstance(images, torch.Tensor) and images.dim() == 3 and images.size(0) < 1:
        raise _lib.GGNNError(shape_text)
    return _image_tensor(images, 3, shape_text, "images")


def grain_offsets(n_grains, device):
    """The union's grain offsets of per-image grain counts: (host list [B + 1], int64 device tensor)."""
    n_grains = [int(n) for n in n_grains]
    if not n_grains or min(n_grains) < 1:
        raise _lib.GGNNError("n_grains must hold one count of at least 1 per image")
    off = np.concatenate([[0], np.cumsum(n_grains, dtype=np.int64)]).astype(np.int64)
    return off.tolist(), torch.from_numpy(off).to(device)


def _vectorize_union(images, n_grains, grid, merge_radius, joint_capacity, boundary="periodic", grain_off=None, extra_words=0,
                     links="unique", max_trace=None, pinch="junction"):
    """`_vectorize` for a stack: every launch, no read-back.  images: what `_stack` returns; grain_off: what `grain_offsets`
    returns (None: formed here, an upload -- pass it to a stream capture).  The status tensor holds the B status rows, behind
    them joint_off [B + 1] and, for no-flux, the 4 B corner pixels: one read-back fetches them all (extra_words: zeroed room
    behind those, for the counters of a caller that wants them in the same read-back).  links="trace": the vectorisation also
    writes `rep`, ggnn_junction_links_trace_traj follows the links call, and its 3 B counters lie behind the corner pixels, at
    v["trace_words"] (None for "unique", whose launches and words are what they were).  pinch="neck": the _pinch_traj entry
    points take the place of their namesakes, and their B counters lie behind everything else, extra_words included, at
    v["pinch_words"] (None for "junction", whose launches and words are what they were)."""
    be = default_backend()
    _check_boundary(boundary)
    _check_pinch(pinch)
    neck = pinch == "neck"
    noflux = boundary == "noflux"
    if grid not in GRIDS:
        raise _lib.GGNNError(f"grid must be 'cells' or 'points', got {grid!r}")
    B, ny, nx = images.shape
    max_trace = _check_links(links, max_trace, nx, ny)
    trace = links == "trace"
    dev = images.device
    if len(n_grains) != B:
        raise _lib.GGNNError("n_grains must hold one count per image")
    off_host, off_dev = grain_offsets(n_grains, dev) if grain_off is None else grain_off
    n_total, R = off_host[-1], int(merge_radius)
    cap = 3 * n_total + 16 * B if joint_capacity is None else int(joint_capacity)
    counts = torch.empty(n_total, dtype=torch.int64, device=dev)       # (zeroed by the call)
    W = _lib.GGNN_JUNCTION_STATUS_WORDS
    trace_words = B * W + B + 1 + (4 * B if noflux else 0) if trace else None
    words = B * W + B + 1 + (4 * B if noflux else 0) + (_lib.GGNN_TRACE_COUNTERS * B if trace else 0) + extra_words
    pinch_words = words if neck else None
    xy, triples, gj, jj, status, ws = _arrays(dev, n_total, cap, B, ny, nx, noflux, words + (B if neck else 0))
    mode, pinched = PINCHES[pinch], (_lib.ptr(status[pinch_words:]) if neck else None)
    if noflux:   # per image, the order of grain_image(corner_grains=)
        status[B * W + B + 1:B * W + 5 * B + 1] = torch.stack([images[:, 0, 0], images[:, 0, -1], images[:, -1, 0], images[:, -1, -1]], 1).reshape(-1)
    off, pitch = GRIDS[grid](nx)
    A = _lib.JunctionTrajArgs()
    A.images, A.grain_off, A.pixel_counts, A.xy = _lib.ptr(images), _lib.ptr(off_dev), _lib.ptr(counts), _lib.ptr(xy)
    A.triples, A.edge_gj, A.status, A.workspace, A.workspace_bytes = (_lib.ptr(triples), _lib.ptr(gj), _lib.ptr(status),
                                                                      _lib.ptr(ws), 4 * ws.numel())
    A.nx, A.ny, A.n_image, A.n_grain, A.joint_capacity = nx, ny, B, n_total, cap
    A.offset, A.pitch, A.merge_radius, A.boundary = float(off), float(pitch), R, BOUNDARIES[boundary]
    rep = None
    if trace:
        rep = torch.zeros(cap, dtype=torch.int32, device=dev)
        if neck:
            _lib.check(be.lib.ggnn_image_junction_windows_pinch_traj(ctypes.byref(A), _lib.ptr(rep), mode, pinched,
                                                                     _lib.current_stream()), "ggnn_image_junction_windows_pinch_traj")
        else:
            _lib.check(be.lib.ggnn_image_junction_windows_traj(ctypes.byref(A), _lib.ptr(rep), _lib.current_stream()),
                       "ggnn_image_junction_windows_traj")
    elif neck:
        _lib.check(be.lib.ggnn_image_junctions_pinch_traj(ctypes.byref(A), mode, pinched, _lib.current_stream()),
                   "ggnn_image_junctions_pinch_traj")
    else:
        _lib.check(be.lib.ggnn_image_junctions_traj(ctypes.byref(A), _lib.current_stream()), "ggnn_image_junctions_traj")
    csr = be.build_csr_batch([(gj.flip(0).contiguous(), cap, n_total + cap)], check=False)[0]
    L = _lib.LinkTrajArgs()
    L.triples, L.rowptr, L.col, L.edge_jj, L.status = (_lib.ptr(triples), _lib.ptr(csr.rowptr), _lib.ptr(csr.col),
                                                       _lib.ptr(jj), _lib.ptr(status))
    L.n_grain, L.joint_capacity, L.E_cap, L.n_image = n_total, cap, csr.col.numel(), B
    _lib.check(be.lib.ggnn_junction_links_traj(ctypes.byref(L), _lib.current_stream()), "ggnn_junction_links_traj")
    T = None
    if trace:
        T = _lib.LinkTraceArgs()
        T.images, T.grain_off, T.triples, T.rep, T.rowptr, T.col = A.images, A.grain_off, L.triples, _lib.ptr(rep), L.rowptr, L.col
        T.edge_jj, T.status, T.counters = L.edge_jj, L.status, _lib.ptr(status[trace_words:])
        T.nx, T.ny, T.n_image, T.n_grain, T.joint_capacity, T.E_cap = nx, ny, B, n_total, cap, L.E_cap
        T.max_trace, T.merge_radius, T.boundary = max_trace, R, BOUNDARIES[boundary]
        if neck:
            _lib.check(be.lib.ggnn_junction_links_trace_pinch_traj(ctypes.byref(T), mode, _lib.current_stream()),
                       "ggnn_junction_links_trace_pinch_traj")
        else:
            _lib.check(be.lib.ggnn_junction_links_trace_traj(ctypes.byref(T), _lib.current_stream()), "ggnn_junction_links_trace_traj")
    return {"xy": xy, "triples": triples, "gj": gj, "jj": jj, "status": status, "counts": counts, "csr": csr,
            "n_grain": n_total, "n_image": B, "grain_off": off_host, "grain_off_dev": off_dev, "capacity": cap,
            "shape": (ny, nx), "boundary": boundary, "max_y": image_max_y(nx, ny, grid) if noflux else None,
            "rep": rep, "trace_words": trace_words, "trace_call": T, "pinch_words": pinch_words, "pinch": pinch,
            "calls": (A, L, images, ws)}


def _graphs(images, n_grains, grid, merge_radius, joint_capacity, strict, boundary="periodic", links="unique", max_trace=None,
            pinch="junction"):
    """graphs_from_images' dict, with the capacity-sized arrays behind it as a second result."""
    _check_boundary(boundary)
    _check_links(links, max_trace, 1, 1)
    _check_pinch(pinch)
    images = _stack(images)
    if n_grains is None:
        n_grains = images.amax(dim=(1, 2)).tolist()   # (a read-back of its own: pass n_grains to avoid it)
    v = _vectorize_union(images, n_grains, grid, merge_radius, joint_capacity, boundary, links=links, max_trace=max_trace,
                         pinch=pinch)
    return _graphs_of(v, v["status"].tolist(), strict)   # the one read-back


def _graphs_of(v, words, strict):
    """`_graphs`' two results from the arrays of `_vectorize_union` and the words of its status, read back."""
    boundary = v["boundary"]
    B, W, cap = v["n_image"], len(STATUS_WORDS), v["capacity"]
    status = [dict(zip(STATUS_WORDS, words[b * W:(b + 1) * W])) for b in range(B)]
    if v.get("trace_words") is not None:   # links="trace": the three counters of every image
        t0, C = v["trace_words"], len(TRACE_COUNTERS)
        for b in range(B):
            status[b].update(zip(TRACE_COUNTERS, words[t0 + C * b:t0 + C * (b + 1)]))
    if v.get("pinch_words") is not None:   # pinch="neck": the pinch windows of every image
        for b in range(B):
            status[b]["n_pinch_windows"] = words[v["pinch_words"] + b]
    joint_off = [min(o, cap) for o in words[B * W:B * W + B + 1]]
    corners = None
    if boundary == "noflux":
        corners = [tuple(words[B * W + B + 1 + 4 * b:B * W + B + 5 + 4 * b]) for b in range(B)]
    v["corner_grains"] = corners
    bad = [b for b in range(B) if not status_is_valid(status[b], boundary)]
    if strict and bad:
        raise ValueError(f"{len(bad)} of {B} images are not valid {boundary} grain structures: "
                         + "; ".join(f"image {b}: {status[b]}" for b in bad)
                         + f" (valid: overflow, n_invalid_pixels and n_open_pairs 0 and {EULER[boundary]}; joint_capacity {cap} "
                           "for the union)")
    xy, triples, ei = _cut(v, joint_off[-1])
    out = {"xy": xy, "triples": triples, "edge_index_dict": ei, "status": status,
           "traj_offsets": {"grain": list(v["grain_off"]), "joint": joint_off}}
    if boundary == "noflux":
        out["corner_grains"], out["max_y"] = corners, v["max_y"]
    return out, v


def graphs_from_images(images, n_grains=None, grid="cells", merge_radius=2, joint_capacity=None, strict=True,
                       boundary="periodic", links="unique", max_trace=None, pinch="junction"):
    """The junction graphs of a stack of grain-ID images as ONE disjoint union: `graph_from_image`'s rule per image, in a
    number of launches that does not depend on the number of images, with one read-back.

    images: integer [B, ny, nx] on the device, or a list of B equal-shaped [ny, nx] device tensors (one shape a stack: the
    project keeps one box per union); n_grains: the B grain counts (None: each image's largest id, at the price of a
    read-back); grid, merge_radius, boundary: as in `graph_from_image`, the same for every image; joint_capacity: room for
    the junctions of the whole union (default 3 sum(n_grains) + 16 B).

    -> dict: `xy` float32 [n_joint, 2], `triples` int32 [n_joint, 3] and `edge_index_dict` (int64 [2, 3 n_joint] per edge
    type) of the union -- image b's grains are traj_offsets["grain"][b] .. and its junctions traj_offsets["joint"][b] ..,
    numbered within the image as `graph_from_image` numbers them --, `status`: a list of B dicts,
    `traj_offsets` = {"grain": [B + 1], "joint": [B + 1]} (host lists, as GrainRollout, enable_events, enable_qoi and
    enable_polygons take them); boundary="noflux": also `corner_grains`, a list of B 4-tuples, and `max_y`.
    `union_member(result, t)` is image t's own graph.

    strict: raise ValueError naming every invalid image and its counters (status_is_valid per image); strict=False returns
    what was found, with -1 as the destination of a joint->joint column whose pair has no partner or more than one.

    links="trace", max_trace: as in `graph_from_image`, per image: every status dict gains n_traced, n_trace_failed and
    n_trace_overflow, and its n_open_pairs is what is still open after tracing.  One more launch and one memset, whatever the
    number of images or of open pairs; still one read-back.

    pinch="neck": as in `graph_from_image`, per image: every status dict gains n_pinch_windows.  The same launches and one
    memset more; still one read-back."""
    return _graphs(images, n_grains, grid, merge_radius, joint_capacity, strict, boundary, links, max_trace, pinch)[0]


def union_member(result, t):
    """Trajectory t of `graphs_from_images`' result with local indices, in the shape of `graph_from_image`'s return value:
    (xy, triples, edge_index_dict, status), for no-flux with (corner_grains, max_y) behind them."""
    og, oj = result["traj_offsets"]["grain"], result["traj_offsets"]["joint"]
    if not 0 <= t < len(og) - 1:
        raise _lib.GGNNError(f"the union has {len(og) - 1} trajectories, got {t}")
    g0, j0, j1 = og[t], oj[t], oj[t + 1]
    ei = result["edge_index_dict"]
    gj = ei[EDGE_TYPES[0]][:, 3 * j0:3 * j1].clone()
    gj[0] -= g0
    gj[1] -= j0
    jj = ei[EDGE_TYPES[2]][:, 3 * j0:3 * j1].clone()
    jj[0] -= j0
    jj[1] = torch.where(jj[1] >= 0, jj[1] - j0, jj[1])
    own = {EDGE_TYPES[0]: gj, EDGE_TYPES[1]: gj.flip(0).contiguous(), EDGE_TYPES[2]: jj}
    out = (result["xy"][j0:j1].contiguous(), result["triples"][j0:j1] - g0, own, result["status"][t])
    if "corner_grains" in result:
        out += (result["corner_grains"][t], result["max_y"])
    return out


def samples_from_images(images, theta_x, theta_z, G, R, span=None, patch_pixels=None, **kw):
    """A union rollout's first state from a stack of grain-ID images: device (x_dict, edge_index_dict, edge_attr,
    traj_offsets), every trajectory's rows being `sample_from_image`'s of its image, bit for bit.

    theta_x, theta_z: lists of B arrays, one angle per grain of the image (their lengths are the grain counts); G, R: scalars
    or length-B sequences, the per-trajectory process columns; span: one value for the union (None: `span_for(G_b, R_b)`,
    which must agree across the images); patch_pixels: as in `sample_from_image`.  The area column comes from the
    per-image pixel counts of the vectorisation, grain centres and edge lengths from one ggnn_grain_centres and one edge
    refresh on the union.  Other keywords go to `graphs_from_images`; an invalid structure always raises.

    boundary="noflux": what `GrainRollout(..., boundary="noflux", traj_offsets=traj_offsets, max_y=image_max_y(nx, ny, grid))`
    takes; the row of every trajectory's boundary grain is reset as `sample_from_image` resets grain 0's."""
    tx = [np.asarray(t, np.float64).ravel() for t in theta_x]
    tz = [np.asarray(t, np.float64).ravel() for t in theta_z]
    B = len(tx)
    if B < 1 or len(tz) != B or any(len(a) != len(b) for a, b in zip(tx, tz)):
        raise _lib.GGNNError("theta_x and theta_z must be lists of one array per image, one angle per grain")
    n_grains = kw.pop("n_grains", None) or [len(t) for t in tx]
    if [int(n) for n in n_grains] != [len(t) for t in tx]:
        raise _lib.GGNNError("theta_x and theta_z must hold one angle per grain")
    Gs, Rs, _, span = _process_columns(B, G, R, None, span, "G and R", "image", "union")
    kw.pop("strict", None)
    boundary = kw.pop("boundary", "periodic")
    res, v = _graphs(images, n_grains, kw.pop("grid", "cells"), kw.pop("merge_radius", 2), kw.pop("joint_capacity", None),
                     True, boundary, kw.pop("links", "unique"), kw.pop("max_trace", None), kw.pop("pinch", "junction"))
    if kw:
        raise TypeError(f"samples_from_images: unknown keywords {sorted(kw)}")
    x, ei, ea = _union_state(res["xy"], res["edge_index_dict"], res["traj_offsets"]["joint"], v, v["counts"],
                             v["grain_off_dev"][:-1], True, tx, tz, Gs, Rs, span, patch_pixels)   # (strict has judged it valid)
    return x, ei, ea, res["traj_offsets"]


def _process_columns(n, G, R, z, span, names, noun, whole):
    """The process columns of n images (or frames: `noun`) of one union (or sequence: `whole`): -> G, R and z (or None) as n
    floats each, and the one frame span (None: `span_for(G_b, R_b)`, which must agree)."""
    from .synthetic import span_for

    def column(c):
        return [float(a) for a in np.broadcast_to(np.asarray(c, np.float64), (n,))]
    try:
        Gs, Rs, zs = column(G), column(R), (None if z is None else column(z))
    except ValueError as exc:
        raise _lib.GGNNError(f"{names} must be scalars or hold one value per {noun}") from exc
    if span is None:
        spans = sorted({span_for(g, r) for g, r in zip(Gs, Rs)})
        if len(spans) != 1:
            raise _lib.GGNNError(f"the {noun}s' (G, R) give the frame spans {spans}: a {whole} has one, pass span=")
        span = spans[0]
    return Gs, Rs, zs, span


def _union_state(xy, ei, joint_off, v, counts, first, valid, tx, tz, Gs, Rs, span, patch_pixels):
    """samples_from_images' (x_dict, edge_index_dict, edge_attr) of a vectorised union: its junctions xy, its edge lists and
    joint offsets; of v its shape, boundary, grains and joint->grain table; counts: the pixels per union grain; first: the
    index of every trajectory's first grain (its boundary grain when there are walls).  Not `valid`: a joint->joint column
    without a destination (strict=False: an invalid image's) is measured as a loop on its source, length 0."""
    from .generator import feature_rows
    be, dev, boundary = default_backend(), xy.device, v["boundary"]
    ny, nx = v["shape"]
    rows = [feature_rows(tx[b], tz[b], joint_off[b + 1] - joint_off[b], Gs[b], Rs[b], span) for b in range(len(tx))]
    x_grain = torch.from_numpy(np.concatenate([fg for fg, _ in rows]).astype(np.float32)).to(dev)
    x_joint = torch.from_numpy(np.concatenate([fj for _, fj in rows]).astype(np.float32)).to(dev)
    x_joint[:, :2] = xy
    x_grain[:, 3] = (counts.to(torch.float64) / float(patch_pixels or nx * ny)).to(torch.float32)
    csr, n_total = v["csr"], v["n_grain"]
    csr_jg = type(csr)(csr.rowptr[:n_total + 1], csr.col, csr.perm, csr.row, csr.unit_ptr, csr.units, csr.E)
    be.grain_centres(csr_jg, x_joint, x_grain, boundary=boundary)
    if boundary == "noflux":   # every trajectory's boundary grain as ggnn_noflux_boundary(_traj) resets it
        x_grain[first, :2] = 0.5
        x_grain[first, 3:5] = 0.0
        x_grain[first, 10] = 0.0
    ea = {et: torch.zeros(ei[et].size(1), 1, dtype=torch.float32, device=dev) for et in EDGE_TYPES}
    x = {"grain": x_grain, "joint": x_joint}
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    measured = dict(ei)
    if not valid:
        jj = ei[EDGE_TYPES[2]]
        measured[EDGE_TYPES[2]] = torch.stack([jj[0], torch.where(jj[1] >= 0, jj[1], jj[0])])
    be.step_refresh(x_joint, x_grain, math.inf, flags,
                    [(measured[et], x[et[0]], x[et[2]], ea[et]) for et in EDGE_TYPES])
    return x, ei, ea


# ---- a recorded sequence into training samples ---------------------------------------------------------------------------

PAIR_COUNTERS = ("n_matched", "n_ambiguous", "n_label0", "n_label1", "n_unlabelled", "n_eliminated")


def _track(frames, n_grain, grid, merge_radius, joint_capacity, boundary, extra_volume=None, patch_pixels=None, targets=True,
           links="unique", max_trace=None, pinch="junction"):
    """Every launch of a tracked sequence, no read-back: `_vectorize_union`'s dict with the frames as its images, plus
    next_joint / prev_joint and, with `targets`, the capacity-sized target arrays.  The counters of ggnn_track_junctions
    [T, 2] and of ggnn_track_targets [T, 4] lie behind the union's status words, at v["counter_words"] (and, with pinch="neck",
    in front of the T pinch counters)."""
    be = default_backend()
    _check_links(links, max_trace, 1, 1)
    _check_pinch(pinch)
    frames = _stack(frames)
    T, ny, nx = frames.shape
    n_grain = int(n_grain)
    if T < 2:
        raise _lib.GGNNError("a sequence needs at least two frames")
    v = _vectorize_union(frames, [n_grain] * T, grid, merge_radius, joint_capacity, boundary, extra_words=6 * T, links=links,
                         max_trace=max_trace, pinch=pinch)
    dev, cap, n_total, csr, status = frames.device, v["capacity"], v["n_grain"], v["csr"], v["status"]
    v["counter_words"] = (status.numel() if v["pinch_words"] is None else v["pinch_words"]) - 6 * T
    counters = status[v["counter_words"]:v["counter_words"] + 6 * T]
    v["next_joint"] = torch.full((cap,), -1, dtype=torch.int64, device=dev)
    v["prev_joint"] = torch.full((cap,), -1, dtype=torch.int64, device=dev)
    K = _lib.TrackArgs()
    K.triples, K.rowptr, K.col, K.grain_off, K.status = (_lib.ptr(v["triples"]), _lib.ptr(csr.rowptr), _lib.ptr(csr.col),
                                                         _lib.ptr(v["grain_off_dev"]), _lib.ptr(status))
    K.next_joint, K.prev_joint, K.counters = _lib.ptr(v["next_joint"]), _lib.ptr(v["prev_joint"]), _lib.ptr(counters)
    K.n_grain, K.joint_capacity, K.E_cap, K.n_frame, K.boundary = n_total, cap, csr.col.numel(), T, BOUNDARIES[boundary]
    _lib.check(be.lib.ggnn_track_junctions(ctypes.byref(K), _lib.current_stream()), "ggnn_track_junctions")
    v["track_calls"] = (K, None)
    if not targets:
        return v
    if extra_volume is not None:
        extra_volume = torch.as_tensor(extra_volume).to(device=dev, dtype=torch.float64).contiguous()
        if extra_volume.shape != (T, n_grain):
            raise _lib.GGNNError("extra_volume must be [T, n_grain]")
    f32 = dict(dtype=torch.float32, device=dev)
    out = {"y_joint": torch.zeros(cap, 2, **f32), "mask_joint": torch.zeros(cap, **f32), "hist_joint": torch.zeros(cap, 2, **f32),
           "edge_label": torch.full((3 * cap,), -1, dtype=torch.int64, device=dev),
           "y_grain": torch.zeros(n_total, 2, **f32), "mask_grain": torch.zeros(n_total, **f32),
           "grain_event": torch.zeros(n_total, dtype=torch.int64, device=dev), "hist_grain": torch.zeros(n_total, 2, **f32)}
    G = _lib.TrackTargetsArgs()
    G.triples, G.rowptr, G.col, G.edge_jj, G.xy = K.triples, K.rowptr, K.col, _lib.ptr(v["jj"]), _lib.ptr(v["xy"])
    G.pixel_counts, G.extra_volume = _lib.ptr(v["counts"]), (None if extra_volume is None else _lib.ptr(extra_volume))
    G.grain_off, G.status, G.next_joint, G.prev_joint = K.grain_off, K.status, K.next_joint, K.prev_joint
    for name, t in out.items():
        setattr(G, name, _lib.ptr(t))
    G.counters, G.patch_pixels = _lib.ptr(counters[2 * T:]), float(patch_pixels or nx * ny)
    G.n_grain, G.joint_capacity, G.E_cap, G.n_frame, G.boundary = n_total, cap, csr.col.numel(), T, BOUNDARIES[boundary]
    _lib.check(be.lib.ggnn_track_targets(ctypes.byref(G), _lib.current_stream()), "ggnn_track_targets")
    v.update(out)
    v["track_calls"] = (K, G, extra_volume)   # (the two calls' arguments and what they point to: tools/vectorize_cost.py)
    return v


def track_frames(frames, n_grain, grid="cells", merge_radius=2, joint_capacity=None, boundary="periodic", links="unique",
                 max_trace=None, pinch="junction"):
    """The frame-to-frame correspondence of a recorded sequence of grain-ID images (ggnn_track_junctions; tests/trackcheck.py
    restates the rule): -> (`graphs_from_images(frames, [n_grain] * T, strict=False)`'s dict, next_joint, prev_joint).

    frames: int [T, ny, nx] on the device or a list of T equal-shaped device images, T >= 2, with grain ids that are stable
    across the frames (pixel p = grain p - 1 in every frame; an eliminated grain no longer occurs).  next_joint int64
    [n_joint]: the union index of the junction of the following frame that carries the same grain triple -- when that triple
    occurs exactly once in both frames, and both frames are valid structures (status_is_valid, judged on the device) --, or
    -1; prev_joint: the same towards the preceding frame, the inverse map.  One read-back, of the status.

    links="trace", max_trace: as in `graphs_from_images`; the frames are traced before they are judged, so a frame with a lens
    or a wall-to-wall band is valid and its pairs are tracked.  The tracker itself is the same: the two junctions of a lens
    share a triple, so they are counted in n_ambiguous and stay unmatched (mask 0), and the links around them are labelled by
    the rule above.

    pinch="neck": as in `graphs_from_images`; the frames are read with it before they are judged, so a frame in which a drifting
    cell edge is a neck through a pixel corner is valid and its pairs are tracked.  The tracker itself is the same."""
    v = _track(frames, n_grain, grid, merge_radius, joint_capacity, boundary, targets=False, links=links, max_trace=max_trace,
               pinch=pinch)
    res, _ = _graphs_of(v, v["status"].tolist(), False)   # the one read-back
    n = res["traj_offsets"]["joint"][-1]
    return res, v["next_joint"][:n].contiguous(), v["prev_joint"][:n].contiguous()


def frames_to_samples(frames, theta_x, theta_z, G, R, span=None, patch_pixels=None, extra_volume=None, z=None, grid="cells",
                      merge_radius=2, joint_capacity=None, boundary="periodic", links="unique", max_trace=None, pinch="junction"):
    """A training set from a recorded sequence of grain-ID images -- a phase-field run, a serial-section series, the
    `grain_images()` of a rollout --: -> (samples, report), one sample per pair of consecutive VALID frames (t, t + 1), each the
    (x, edge_index, edge_attr, y, mask) of device tensors with local indices that `training.DeviceDataset` takes.  What the
    reference gets from its junction tracker (graph_trajectory.py:283-846) and form_gradient (graph_datastruct.py:851-1011).

    frames: as in `track_frames`; theta_x, theta_z: one angle per grain (n_grain = their length, the same in every frame;
    boundary="noflux": they count the boundary grain, grain 0); G, R: scalars or one value per frame; span, patch_pixels: as in
    `samples_from_images`; extra_volume: float [T, n_grain], the reference's extraV_frames[:, frame] / s**3, a solver output
    that the frames do not hold (None: zeros); z: [T], the z feature of every row of a frame (None: 0).

    x, edge_index, edge_attr of sample t are frame t's rows of `samples_from_images(frames, ...)` bit for bit (the frames are
    vectorised with strict=False: an invalid frame is skipped with its pairs, not raised), except the history columns:
    x_grain[:, 4] = fp32(20 extra_volume[t]), and, when the pair (t - 1, t) was emitted too, x_grain[:, 10] = the area change
    and x_joint[:, 6:8] = the displacement since frame t - 1 in the targets' scaling (0 for a first sample, after a skipped
    pair and for a junction without a predecessor; the row of a grain without pixels in frame t keeps only its orientation, span
    and process columns).  y = {"grain": [n_grain, 2] (20 x the change of the area feature; 20 x
    extra_volume[t + 1]), "joint": [n_joint_t, 2] (5 x the displacement to the matched junction; periodic: its minimum
    image), "edge_event": int64 [3 n_joint_t] (0: the link persists, 1: a neighbour switch, -1: unlabelled), "grain_event":
    int64 [n_grain] (1: the grain has pixels in frame t and none in t + 1)}; mask = {"grain": [n_grain, 1], "joint":
    [n_joint_t, 1]} float32 (a grain with pixels in frame t; a matched junction).  include/ggnn.h states the rule in full.

    report = {"status": per frame, "pairs": [(t, t + 1)] emitted, "skipped": [(t, t + 1, reason)], "counts": per emitted pair
    a dict of n_matched, n_ambiguous, n_label0, n_label1, n_unlabelled, n_eliminated}.  Everything is found on the device
    (ggnn_track_junctions, ggnn_track_targets) in a number of launches that does not depend on T, with ONE read-back: the
    union's status words and the counters behind them.  Cutting the union into samples is a slice per pair.

    links="trace", max_trace: as in `graphs_from_images`: the frames are traced on the device before the tracker judges them, so
    the frame in which a grain is a lens on a boundary, one frame before it vanishes, is valid and keeps its two pairs -- the
    ones that carry the classifier's positive labels; report["status"] carries n_traced, n_trace_failed and n_trace_overflow
    per frame.  The tracker itself is the same: the two junctions of a lens share a triple, so they are counted in n_ambiguous
    and stay unmatched (mask 0), and the links around them are labelled by the rule above.

    pinch="neck": as in `graphs_from_images`: a frame in which a drifting cell edge is a neck through a pixel corner is read as
    the valid structure it is and keeps its two pairs, with no pixel changed and no grain renumbered; report["status"] carries
    n_pinch_windows per frame and report["n_pinch_windows"] lists them.  The tracker itself is the same.  With the default the
    report is what it was."""
    tx, tz = np.asarray(theta_x, np.float64).ravel(), np.asarray(theta_z, np.float64).ravel()
    n_grain = len(tx)
    if n_grain < 1 or len(tz) != n_grain:
        raise _lib.GGNNError("theta_x and theta_z must hold one angle per grain")
    _check_boundary(boundary)
    _check_links(links, max_trace, 1, 1)
    _check_pinch(pinch)
    frames = _stack(frames)
    T = frames.size(0)
    Gs, Rs, zs, span = _process_columns(T, G, R, z, span, "G, R and z", "frame", "sequence")
    v = _track(frames, n_grain, grid, merge_radius, joint_capacity, boundary, extra_volume, patch_pixels, links=links,
               max_trace=max_trace, pinch=pinch)
    words = v["status"].tolist()                      # the one read-back
    res, _ = _graphs_of(v, words, False)
    oj, n = res["traj_offsets"]["joint"], res["traj_offsets"]["joint"][-1]
    valid = [status_is_valid(s, boundary) for s in res["status"]]
    x, ei, ea = _union_state(res["xy"], res["edge_index_dict"], oj, v, v["counts"], v["grain_off_dev"][:-1], all(valid),
                             [tx] * T, [tz] * T, Gs, Rs, span, patch_pixels)
    x["grain"][:, 4] = v["hist_grain"][:, 1]
    x["grain"][:, 10] = v["hist_grain"][:, 0]
    x["joint"][:, 6:8] = v["hist_joint"][:n]
    if zs is not None:
        for t in range(T):
            x["grain"][t * n_grain:(t + 1) * n_grain, 2] = zs[t]
            x["joint"][oj[t]:oj[t + 1], 2] = zs[t]
    c0 = v["counter_words"]
    report = {"status": res["status"], "pairs": [], "skipped": [], "counts": []}
    if pinch == "neck":
        report["n_pinch_windows"] = [s["n_pinch_windows"] for s in res["status"]]
    samples = []
    for t in range(T - 1):
        if not (valid[t] and valid[t + 1]):
            bad = [u for u in (t, t + 1) if not valid[u]]
            report["skipped"].append((t, t + 1, "; ".join(f"frame {u} is not a valid {boundary} structure: {res['status'][u]}"
                                                          for u in bad)))
            continue
        g0, g1, j0, j1 = t * n_grain, (t + 1) * n_grain, oj[t], oj[t + 1]
        own = union_member(res, t)[2]
        sx = {"grain": x["grain"][g0:g1].clone(), "joint": x["joint"][j0:j1].clone()}
        sea = {EDGE_TYPES[0]: ea[EDGE_TYPES[0]][3 * j0:3 * j1].clone(), EDGE_TYPES[1]: ea[EDGE_TYPES[1]][3 * j0:3 * j1].clone(),
               EDGE_TYPES[2]: ea[EDGE_TYPES[2]][3 * j0:3 * j1].clone()}
        y = {"grain": v["y_grain"][g0:g1].clone(), "joint": v["y_joint"][j0:j1].clone(),
             "edge_event": v["edge_label"][3 * j0:3 * j1].clone(), "grain_event": v["grain_event"][g0:g1].clone()}
        mask = {"grain": v["mask_grain"][g0:g1].reshape(-1, 1).clone(), "joint": v["mask_joint"][j0:j1].reshape(-1, 1).clone()}
        samples.append((sx, own, sea, y, mask))
        report["pairs"].append((t, t + 1))
        a, b = words[c0 + 2 * t:c0 + 2 * t + 2], words[c0 + 2 * T + 4 * t:c0 + 2 * T + 4 * t + 4]
        report["counts"].append(dict(zip(PAIR_COUNTERS, a + b)))
    return samples, report


# ---- a measured map into a grain-ID image --------------------------------------------------------------------------------

LABEL_STATUS_WORDS = ("n_components", "n_specks", "n_speck_pixels", "n_invalid_in", "n_grains", "n_sweeps", "n_unfilled",
                      "overflow", "n_bound_hits")


def _label_mask(valid, shape, text):
    """The optional mask of a labelling call as contiguous bytes; shape: the map's, or the stack's."""
    if valid is None:
        return None
    if not isinstance(valid, torch.Tensor) or not valid.is_cuda or valid.shape != tuple(shape):
        raise _lib.GGNNError(f"valid must be a {text} device mask")
    return (valid != 0).to(torch.uint8).contiguous()


def _label_cleanup(ny, nx, min_pixels, max_sweeps, grain_capacity):
    """min_pixels, max_sweeps and the rows per map of a labelling call, checked."""
    min_pixels, max_sweeps = int(min_pixels), int(max_sweeps)
    if min_pixels < 1:
        raise _lib.GGNNError("min_pixels must be at least 1")
    if not 0 <= max_sweeps <= _lib.GGNN_LABEL_MAX_SWEEPS:
        raise _lib.GGNNError(f"max_sweeps must lie in [0, {_lib.GGNN_LABEL_MAX_SWEEPS}]")
    cap = ny * nx // min_pixels + 2 if grain_capacity is None else int(grain_capacity)
    if cap < 1:
        raise _lib.GGNNError("grain_capacity must be at least 1")
    return min_pixels, max_sweeps, cap


def _label_inputs(ids, angles, tol, valid, boundary, stack):
    """What `_label` (one map) and `_label_stack` (stack: a leading T) check of their inputs: -> (ids, angles, valid) as the
    library takes them, K, and the shape of ids (of angles without K)."""
    _check_boundary(boundary)
    if (ids is None) == (angles is None):
        raise _lib.GGNNError("exactly one of ids and angles must be given")
    src = ids if angles is None else angles
    if not isinstance(src, torch.Tensor) or not src.is_cuda:
        raise _lib.GGNNError("ids / angles must be device tensors")
    lead, dims = ("[T, ", 3) if stack else ("[", 2)
    if angles is None:
        if ids.dim() != dims or ids.dtype not in (torch.int16, torch.int32, torch.int64, torch.uint8, torch.int8):
            raise _lib.GGNNError(f"ids must be an integer {lead}ny, nx] device tensor")
        ids = ids.to(torch.int32).contiguous()
        K, shape = 0, tuple(ids.shape)
    else:
        if tol is None:
            raise _lib.GGNNError("angles need tol, the largest difference per channel that still links two neighbours")
        if angles.dim() != dims + 1 or not 1 <= angles.size(-3) <= 4 or angles.dtype != torch.float32:
            raise _lib.GGNNError(f"angles must be a float32 {lead}K, ny, nx] device tensor with 1 <= K <= 4")
        angles = angles.contiguous()
        K, shape = angles.size(-3), tuple(angles.shape[:-3]) + tuple(angles.shape[-2:])
    if shape[-1] < 3 or shape[-2] < 3:
        raise _lib.GGNNError("the image must have at least 3 x 3 pixels")
    if stack and shape[0] < 1:
        raise _lib.GGNNError("a stack holds at least one map")
    return ids, angles, _label_mask(valid, shape, f"{lead}ny, nx]"), K, shape


def _label(ids, angles, tol, valid, min_pixels, max_sweeps, boundary, grain_capacity):
    """Every launch of `label_grains`, no read-back: -> dict of the image, the capacity-sized means (None with ids), the
    status words on the device, and the call's arguments with what they point to (tools/vectorize_cost.py)."""
    be = default_backend()
    ids, angles, valid, K, (ny, nx) = _label_inputs(ids, angles, tol, valid, boundary, False)
    dev = (ids if angles is None else angles).device
    min_pixels, max_sweeps, cap = _label_cleanup(ny, nx, min_pixels, max_sweeps, grain_capacity)
    image = torch.empty(ny, nx, dtype=torch.int32, device=dev)
    means = torch.zeros(K, cap, dtype=torch.float32, device=dev) if K else None
    status = torch.empty(_lib.GGNN_LABEL_STATUS_WORDS, dtype=torch.int64, device=dev)   # (zeroed by the call)
    ws = torch.empty(be.lib.ggnn_label_workspace_bytes(nx, ny, K), dtype=torch.uint8, device=dev)
    A = _lib.LabelArgs()
    A.ids, A.angles, A.valid, A.image, A.mean_angles = _lib.ptr(ids), _lib.ptr(angles), _lib.ptr(valid), _lib.ptr(image), _lib.ptr(means)
    A.status, A.workspace, A.workspace_bytes = _lib.ptr(status), _lib.ptr(ws), ws.numel()
    A.nx, A.ny, A.grain_capacity, A.min_pixels = nx, ny, cap, min_pixels
    A.tol, A.K, A.max_sweeps, A.boundary = (0.0 if tol is None else float(np.float32(tol))), K, max_sweeps, BOUNDARIES[boundary]
    _lib.check(be.lib.ggnn_label_grains(ctypes.byref(A), _lib.current_stream()), "ggnn_label_grains")
    return {"image": image, "means": means, "status": status, "capacity": cap, "boundary": boundary,
            "calls": (A, ids, angles, valid, ws)}


def _stack_workspace(need, T, ny, nx):
    """The scratch of a stacked labelling call of `need` bytes (0: the library takes no such stack)."""
    if need == 0:
        raise _lib.GGNNError(f"a stack of {T} maps of {ny} x {nx} pixels is beyond what one labelling call takes (T ny nx <= "
                             f"{2 ** 31 - 1}, nx and ny below {1 << 15}): split it")
    return need


def _label_stack(ids, angles, tol, valid, min_pixels, max_sweeps, boundary, grain_capacity):
    """Every launch of `label_maps` (ggnn_label_grains_stack), no read-back: `_label`'s dict with stacked tensors -- the images
    [T, ny, nx], the capacity-sized means [T, K, capacity] (None with ids), the status words [T, 9] on the device."""
    be = default_backend()
    ids, angles, valid, K, (T, ny, nx) = _label_inputs(ids, angles, tol, valid, boundary, True)
    dev = (ids if angles is None else angles).device
    min_pixels, max_sweeps, cap = _label_cleanup(ny, nx, min_pixels, max_sweeps, grain_capacity)
    need = _stack_workspace(be.lib.ggnn_label_stack_workspace_bytes(T, nx, ny, K), T, ny, nx)
    image = torch.empty(T, ny, nx, dtype=torch.int32, device=dev)
    means = torch.zeros(T, K, cap, dtype=torch.float32, device=dev) if K else None
    status = torch.empty(T, _lib.GGNN_LABEL_STATUS_WORDS, dtype=torch.int64, device=dev)   # (zeroed by the call)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    A = _lib.LabelStackArgs()
    A.ids, A.angles, A.valid, A.image, A.mean_angles = _lib.ptr(ids), _lib.ptr(angles), _lib.ptr(valid), _lib.ptr(image), _lib.ptr(means)
    A.status, A.workspace, A.workspace_bytes = _lib.ptr(status), _lib.ptr(ws), ws.numel()
    A.T, A.nx, A.ny, A.grain_capacity, A.min_pixels = T, nx, ny, cap, min_pixels
    A.tol, A.K, A.max_sweeps, A.boundary = (0.0 if tol is None else float(np.float32(tol))), K, max_sweeps, BOUNDARIES[boundary]
    _lib.check(be.lib.ggnn_label_grains_stack(ctypes.byref(A), _lib.current_stream()), "ggnn_label_grains_stack")
    return {"image": image, "means": means, "status": status, "capacity": cap, "boundary": boundary,
            "calls": (A, ids, angles, valid, ws)}


def _stack_statuses(v, words, entry):
    """The status rows of a stacked labelling, read back as `words` -> (n_grains, statuses), a count and a dict per map; raises
    on a parent walk that reached its bound and names the map."""
    n = len(LABEL_STATUS_WORDS)
    statuses = [dict(zip(LABEL_STATUS_WORDS, words[n * t:n * t + n])) for t in range(v["image"].size(0))]
    for t, s in enumerate(statuses):
        if s["n_bound_hits"]:
            raise _lib.GGNNError(f"{entry}: frame {t}: {s['n_bound_hits']} threads reached the bound of a parent walk: {s}")
    noflux = 1 if v["boundary"] == "noflux" else 0
    return [s["n_grains"] + noflux for s in statuses], statuses


def label_maps(ids=None, angles=None, tol=None, valid=None, min_pixels=1, max_sweeps=64, boundary="periodic", grain_capacity=None):
    """`label_grains` for a STACK of T equal-shaped maps -- a recorded sequence, or an ensemble of scans for one union rollout
    -- in the launches of one map (ggnn_label_grains_stack): every map comes out bit for bit as `label_grains`
    gives it alone.  Maps never interact: the periodic wrap of a map goes to its own first row and column.

    Exactly one of ids -- integer [T, ny, nx] -- and angles -- float32 [T, K, ny, nx] with tol --, on the device; valid: an
    optional [T, ny, nx] mask; min_pixels, max_sweeps, boundary: as in `label_grains`, the same for every map; grain_capacity:
    rows PER MAP (default ny nx // min_pixels + 2, which cannot overflow).

    -> (images int32 [T, ny, nx], n_grains: a list of T ints, mean_angles float32 [T, K, capacity] or None with ids, statuses: a
    list of T dicts as `label_grains` gives them).  Ids restart in every map; map t's means are mean_angles[t, :, :n_grains[t]],
    the rows beyond are zero.  Device tensors in, device tensors out, ONE read-back (the T status rows); two memsets and
    9 + 2 max_sweeps launches whatever T.  Raises on a non-zero n_bound_hits and names the map.

    Not covered: stacks of mixed shapes, and stacks of more than 2^31 - 1 pixels: the caller splits those."""
    v = _label_stack(ids, angles, tol, valid, min_pixels, max_sweeps, boundary, grain_capacity)
    n_grains, statuses = _stack_statuses(v, v["status"].reshape(-1).tolist(), "ggnn_label_grains_stack")   # the one read-back
    return v["image"], n_grains, v["means"], statuses


def label_grains(ids=None, angles=None, tol=None, valid=None, min_pixels=1, max_sweeps=64, boundary="periodic",
                 grain_capacity=None):
    """Segment a measured map into a grain-ID image on the device (ggnn_label_grains; include/ggnn.h states the rule,
    tests/labelcheck.py restates it): connected components of the pixel-to-pixel links, specks and non-indexed
    pixels dissolved into their neighbours, canonical numbering, per-grain mean angles.

    Exactly one of ids -- integer [ny, nx] on the device, a pixel is valid when id >= 1, two 4-neighbours are linked when their
    ids are equal -- and angles -- float32 [K, ny, nx] on the device, 1 <= K <= 4 (K = 2: theta_x, theta_z in radians), a pixel
    is valid when every channel is finite with |a| <= 8, two 4-neighbours are linked when |a_k - b_k| <= tol in every channel
    (tol is required; the pixel-to-pixel misorientation criterion, not transitive).  valid: an optional [ny, nx] device mask,
    0 = non-indexed.  min_pixels: a component with fewer pixels is a speck; specks and invalid pixels are dissolved into the
    neighbouring grains by majority in at most max_sweeps Jacobi sweeps (1: nothing valid is cleaned up).  boundary: "periodic"
    (neighbours wrap; ids from 1) or "noflux" (walls; ids from 2, id 1 being the boundary grain of `graph_from_image`).
    grain_capacity: room of the per-grain rows (default ny nx // min_pixels + 2, which cannot overflow).

    -> (image int32 [ny, nx], n_grain, mean_angles float32 [K, n_grain] or None with ids, status dict): grains numbered in raster
    order of their first pixel, 0 = a pixel no sweep reached (`graph_from_image` counts it in n_invalid_pixels); the means run
    over the pixels of the original components only.  status: n_components, n_specks, n_speck_pixels, n_invalid_in, n_grains,
    n_sweeps, n_unfilled, overflow (more grains than grain_capacity: the image is complete, the means hold the first rows).
    Device tensors in, device tensors out, ONE read-back (the status); 9 + 2 max_sweeps launches whatever the image holds.

    A stack of equal-shaped maps in the same launches is `label_maps` (`label_sequence` also gives a sequence's grains the ids
    that persist across the frames, which `frames_to_samples` needs).  Not covered: 8-connectivity.  The per-channel rule knows no crystal
    symmetry: Euler-angle triples or quaternions under cubic symmetry are `label_orientations`."""
    v = _label(ids, angles, tol, valid, min_pixels, max_sweeps, boundary, grain_capacity)
    status = dict(zip(LABEL_STATUS_WORDS, v["status"].tolist()))   # the one read-back
    if status["n_bound_hits"]:
        raise _lib.GGNNError(f"ggnn_label_grains: {status['n_bound_hits']} threads reached the bound of a parent walk: {status}")
    n_grain = status["n_grains"] + (1 if boundary == "noflux" else 0)
    means = None if v["means"] is None else v["means"][:, :min(n_grain, v["capacity"])].contiguous()
    return v["image"], n_grain, means, status


def sample_from_orientations(theta_x_map, theta_z_map, G, R, tol, min_pixels=1, **kw):
    """A rollout's first state from an orientation map: `label_grains` on the two angle maps ([ny, nx] float32 on the device,
    radians), the per-grain mean angles read back, and `sample_from_image` on the labelled image with everything it takes
    (span, patch_pixels, grid, merge_radius, boundary, links, ...); valid, max_sweeps and grain_capacity go to `label_grains`.

    -> (x_dict, edge_index_dict, edge_attr, image, status): the first three are bit for bit what
    `sample_from_image(image, theta_x, theta_z, ...)` gives on the returned image and the labelling's mean angles (no-flux: row
    0, the boundary grain's, is 0); status is the labelling's, with the means under "theta_x" and "theta_z" (host float32).  A
    map whose labelled image is no valid structure raises, as `sample_from_image` does."""
    if not isinstance(theta_x_map, torch.Tensor) or not isinstance(theta_z_map, torch.Tensor) or theta_x_map.shape != theta_z_map.shape:
        raise _lib.GGNNError("theta_x_map and theta_z_map must be equal-shaped [ny, nx] device tensors")
    boundary = kw.get("boundary", "periodic")
    label_kw = {k: kw.pop(k) for k in ("valid", "max_sweeps", "grain_capacity") if k in kw}
    angles = torch.stack([theta_x_map.to(torch.float32), theta_z_map.to(torch.float32)])
    image, n_grain, means, status = label_grains(angles=angles, tol=tol, min_pixels=min_pixels, boundary=boundary, **label_kw)
    if status["overflow"]:
        raise ValueError(f"the map has more grains than grain_capacity: {status}")
    theta = means.cpu().numpy()
    x, ei, ea = sample_from_image(image, theta[0], theta[1], G, R, n_grain=n_grain, **kw)
    return x, ei, ea, image, dict(status, theta_x=theta[0], theta_z=theta[1])


def _no_map_overflows(statuses):
    """Raises on the first map of a labelled stack that has more grains than rows, and names it."""
    for t, s in enumerate(statuses):
        if s["overflow"]:
            raise ValueError(f"map {t} has more grains than grain_capacity: {s}")


def _union_from_labelled(images, n_grains, statuses, theta, G, R, kw):
    """`samples_from_images` on a labelled stack: theta, a (theta_x, theta_z) pair of host arrays per map -> what
    `samples_from_orientation_maps` returns."""
    x, ei, ea, traj_offsets = samples_from_images(images, [a for a, _ in theta], [b for _, b in theta], G, R, n_grains=n_grains, **kw)
    statuses = [dict(s, theta_x=a, theta_z=b) for s, (a, b) in zip(statuses, theta)]
    return x, ei, ea, traj_offsets, images, statuses


def samples_from_orientation_maps(theta_x_maps, theta_z_maps, G, R, tol, min_pixels=1, **kw):
    """A union rollout's first state from a stack of orientation maps (an ensemble of scans): `label_maps` on the two stacks of
    angle maps ([T, ny, nx] float32 on the device, radians), the per-grain mean angles read back once, and
    `samples_from_images` on the labelled images with everything it takes (span, patch_pixels, grid, merge_radius,
    joint_capacity, boundary, links, max_trace; G and R: scalars or one value per map); valid, max_sweeps and grain_capacity
    go to `label_maps`.

    -> (x_dict, edge_index_dict, edge_attr, traj_offsets, images, statuses): the first four as `samples_from_images` gives
    them -- every trajectory's rows are, bit for bit, `sample_from_orientations`' on that map alone --; images int32
    [T, ny, nx]; statuses: per map the labelling's status with the means under "theta_x" and "theta_z" (host float32).  Three
    read-backs whatever T: the label status, the means, the vectoriser's status.  A map that overflows grain_capacity raises
    and is named; a map whose labelled image is no valid structure raises, as `samples_from_images` does.  One shape a stack."""
    if (not isinstance(theta_x_maps, torch.Tensor) or not isinstance(theta_z_maps, torch.Tensor) or theta_x_maps.dim() != 3
            or theta_x_maps.shape != theta_z_maps.shape):
        raise _lib.GGNNError("theta_x_maps and theta_z_maps must be equal-shaped [T, ny, nx] device tensors")
    label_kw = {k: kw.pop(k) for k in ("valid", "max_sweeps", "grain_capacity") if k in kw}
    angles = torch.stack([theta_x_maps.to(torch.float32), theta_z_maps.to(torch.float32)], 1)
    images, n_grains, means, statuses = label_maps(angles=angles, tol=tol, min_pixels=min_pixels, boundary=kw.get("boundary", "periodic"),
                                                   **label_kw)
    _no_map_overflows(statuses)
    host = means[:, :, :max(n_grains)].cpu().numpy()                       # every map's rows in one read-back
    theta = [(host[t, 0, :n].copy(), host[t, 1, :n].copy()) for t, n in enumerate(n_grains)]
    return _union_from_labelled(images, n_grains, statuses, theta, G, R, kw)


# ---- a measured map of full orientations under crystal symmetry ---------------------------------------------------------

SYMMETRIES = {"none": _lib.GGNN_SYM_NONE, "cubic": _lib.GGNN_SYM_CUBIC}


def quaternions_from_bunge(phi1, Phi, phi2, degrees=False):
    """Bunge Euler angles (phi1, Phi, phi2: equal-shaped tensors or arrays, [ny, nx] or [T, ny, nx]) -> the unit quaternions
    float32 [4, ny, nx] (or [T, 4, ny, nx]) that `label_orientations` takes: crystal to sample, Rz(phi1) Rx(Phi) Rz(phi2), formed
    in fp64 and rounded once:  w = cos(Phi/2) cos((phi1+phi2)/2), x = sin(Phi/2) cos((phi1-phi2)/2), y = sin(Phi/2)
    sin((phi1-phi2)/2), z = cos(Phi/2) sin((phi1+phi2)/2).  The result lies where the inputs lie."""
    a, B, c = (torch.as_tensor(v).to(torch.float64) for v in (phi1, Phi, phi2))
    if a.shape != B.shape or a.shape != c.shape:
        raise _lib.GGNNError("phi1, Phi and phi2 must be equal-shaped")
    if degrees:
        a, B, c = (torch.deg2rad(v) for v in (a, B, c))
    half, plus, minus = B / 2, (a + c) / 2, (a - c) / 2
    q = [torch.cos(half) * torch.cos(plus), torch.sin(half) * torch.cos(minus), torch.sin(half) * torch.sin(minus),
         torch.cos(half) * torch.sin(plus)]
    return torch.stack(q, max(a.dim() - 2, 0)).to(torch.float32).contiguous()


def growth_angles(mean_quats):
    """The model's per-grain angles from orientations: mean_quats [4, n] (a tensor or an array; crystal to sample, normalised
    here) -> (theta_x, theta_z) float64 [n], of the input's kind.  The six directions +c0, +c1, +c2, -c0, -c1, -c2, c_j the
    columns of R(q), are the crystal's <100> axes in the sample frame; u is the one with the largest z component (the first on a
    tie): the preferred growth direction nearest the sample's z.  theta_x = arctan2(u_y, u_x) % (pi/2), theta_z =
    arctan2(hypot(u_x, u_y), u_z) <= 54.74 degrees, as the reference derives them from its drawn direction.  Equal for the 24
    cubic equivalents of one orientation.  fp64 on the host: a row a grain, no hot path."""
    as_tensor = isinstance(mean_quats, torch.Tensor)
    q = (mean_quats.detach().cpu().numpy() if as_tensor else np.asarray(mean_quats)).astype(np.float64)
    if q.ndim != 2 or q.shape[0] != 4:
        raise _lib.GGNNError("mean_quats must be [4, n]")
    w, x, y, z = q / np.sqrt((q * q).sum(0))
    cols = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)]),
                     np.stack([2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)]),
                     np.stack([2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)])])   # [column, component, n]
    six = np.concatenate([cols, -cols])
    u = six[np.argmax(six[:, 2], 0), :, np.arange(q.shape[1])]                                         # [n, 3]
    theta_x, theta_z = np.arctan2(u[:, 1], u[:, 0]) % (np.pi / 2), np.arctan2(np.hypot(u[:, 0], u[:, 1]), u[:, 2])
    if as_tensor:
        return torch.from_numpy(theta_x).to(mean_quats.device), torch.from_numpy(theta_z).to(mean_quats.device)
    return theta_x, theta_z


def _orient_inputs(quats, tol, valid, boundary, symmetry, stack):
    """What `_label_orient` (one map) and `_label_orient_stack` (stack: a leading T) check of their inputs: -> (quats, valid) as
    the library takes them, cos(tol / 2), and the shape of the map or of the stack."""
    _check_boundary(boundary)
    if symmetry not in SYMMETRIES:
        raise _lib.GGNNError(f"symmetry must be one of {sorted(SYMMETRIES)}")
    if tol is None or not 0.0 < float(tol) < math.pi / 2:
        raise _lib.GGNNError("tol, the largest disorientation in radians that still links two neighbours, must lie in (0, pi/2)")
    cos_half_tol = float(np.float32(np.cos(np.float64(tol) / 2)))                       # the one number formed on the host
    if not cos_half_tol > float(np.float32(_lib.GGNN_ORIENT_H)):
        raise _lib.GGNNError(f"tol {tol} is pi/2 to float32: cos(tol / 2) rounds to {cos_half_tol}, which the library refuses")
    lead, dims = ("[T, ", 4) if stack else ("[", 3)
    if (not isinstance(quats, torch.Tensor) or not quats.is_cuda or quats.dim() != dims or quats.size(-3) != 4 or quats.dtype != torch.float32
            or (stack and quats.size(0) < 1)):
        raise _lib.GGNNError(f"quats must be a float32 {lead}4, ny, nx] device tensor")
    quats = quats.contiguous()
    shape = tuple(quats.shape[:-3]) + tuple(quats.shape[-2:])
    if shape[-1] < 3 or shape[-2] < 3:
        raise _lib.GGNNError("the map must have at least 3 x 3 pixels")
    return quats, _label_mask(valid, shape, f"{lead}ny, nx]"), cos_half_tol, shape


def _label_orient(quats, tol, valid, min_pixels, max_sweeps, boundary, grain_capacity, symmetry):
    """Every launch of `label_orientations`, no read-back: -> dict of the image, the capacity-sized mean quaternions, the status
    words on the device, and the call's arguments with what they point to (tools/vectorize_cost.py)."""
    be = default_backend()
    quats, valid, cos_half_tol, (ny, nx) = _orient_inputs(quats, tol, valid, boundary, symmetry, False)
    dev = quats.device
    min_pixels, max_sweeps, cap = _label_cleanup(ny, nx, min_pixels, max_sweeps, grain_capacity)
    image = torch.empty(ny, nx, dtype=torch.int32, device=dev)
    means = torch.zeros(4, cap, dtype=torch.float32, device=dev)
    status = torch.empty(_lib.GGNN_LABEL_STATUS_WORDS, dtype=torch.int64, device=dev)   # (zeroed by the call)
    ws = torch.empty(be.lib.ggnn_label_orient_workspace_bytes(nx, ny), dtype=torch.uint8, device=dev)
    A = _lib.LabelOrientArgs()
    A.quats, A.valid, A.image, A.mean_quats = _lib.ptr(quats), _lib.ptr(valid), _lib.ptr(image), _lib.ptr(means)
    A.status, A.workspace, A.workspace_bytes = _lib.ptr(status), _lib.ptr(ws), ws.numel()
    A.nx, A.ny, A.grain_capacity, A.min_pixels = nx, ny, cap, min_pixels
    A.cos_half_tol = cos_half_tol
    A.symmetry, A.max_sweeps, A.boundary = SYMMETRIES[symmetry], max_sweeps, BOUNDARIES[boundary]
    _lib.check(be.lib.ggnn_label_orientations(ctypes.byref(A), _lib.current_stream()), "ggnn_label_orientations")
    return {"image": image, "means": means, "status": status, "capacity": cap, "boundary": boundary,
            "calls": (A, quats, valid, ws)}


def _label_orient_stack(quats, tol, valid, min_pixels, max_sweeps, boundary, grain_capacity, symmetry):
    """Every launch of `label_orientation_maps` (ggnn_label_orientations_stack), no read-back: `_label_orient`'s dict with
    stacked tensors -- the images [T, ny, nx], the mean quaternions [T, 4, capacity], the status words [T, 9] on the device."""
    be = default_backend()
    quats, valid, cos_half_tol, (T, ny, nx) = _orient_inputs(quats, tol, valid, boundary, symmetry, True)
    dev = quats.device
    min_pixels, max_sweeps, cap = _label_cleanup(ny, nx, min_pixels, max_sweeps, grain_capacity)
    need = _stack_workspace(be.lib.ggnn_label_orient_stack_workspace_bytes(T, nx, ny), T, ny, nx)
    image = torch.empty(T, ny, nx, dtype=torch.int32, device=dev)
    means = torch.zeros(T, 4, cap, dtype=torch.float32, device=dev)
    status = torch.empty(T, _lib.GGNN_LABEL_STATUS_WORDS, dtype=torch.int64, device=dev)   # (zeroed by the call)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    A = _lib.LabelOrientStackArgs()
    A.quats, A.valid, A.image, A.mean_quats = _lib.ptr(quats), _lib.ptr(valid), _lib.ptr(image), _lib.ptr(means)
    A.status, A.workspace, A.workspace_bytes = _lib.ptr(status), _lib.ptr(ws), ws.numel()
    A.T, A.nx, A.ny, A.grain_capacity, A.min_pixels = T, nx, ny, cap, min_pixels
    A.cos_half_tol = cos_half_tol
    A.symmetry, A.max_sweeps, A.boundary = SYMMETRIES[symmetry], max_sweeps, BOUNDARIES[boundary]
    _lib.check(be.lib.ggnn_label_orientations_stack(ctypes.byref(A), _lib.current_stream()), "ggnn_label_orientations_stack")
    return {"image": image, "means": means, "status": status, "capacity": cap, "boundary": boundary,
            "calls": (A, quats, valid, ws)}


def label_orientation_maps(quats, tol, valid=None, min_pixels=1, max_sweeps=64, boundary="periodic", grain_capacity=None,
                           symmetry="cubic"):
    """`label_orientations` for a STACK of T equal-shaped maps in the launches of one map (ggnn_label_orientations_stack; DESIGN
    8r): every map comes out bit for bit as `label_orientations` gives it alone; the alignment target of a grain's mean is the
    first pixel of its component in its own map.

    quats: float32 [T, 4, ny, nx] on the device; valid: an optional [T, ny, nx] mask; everything else as in
    `label_orientations`, the same for every map; grain_capacity: rows PER MAP.

    -> (images int32 [T, ny, nx], n_grains: a list of T ints, mean_quats float32 [T, 4, capacity], statuses: a list of T dicts):
    map t's means are mean_quats[t, :, :n_grains[t]], the rows beyond are zero.  ONE read-back (the T status rows); two
    memsets and 12 + 2 max_sweeps launches whatever T.  Raises on a non-zero n_bound_hits and names the map.

    Not covered: stacks of mixed shapes, and stacks of more than 2^31 - 1 pixels: the caller splits those."""
    v = _label_orient_stack(quats, tol, valid, min_pixels, max_sweeps, boundary, grain_capacity, symmetry)
    n_grains, statuses = _stack_statuses(v, v["status"].reshape(-1).tolist(), "ggnn_label_orientations_stack")   # the one read-back
    return v["image"], n_grains, v["means"], statuses


def label_orientations(quats, tol, valid=None, min_pixels=1, max_sweeps=64, boundary="periodic", grain_capacity=None,
                       symmetry="cubic"):
    """Segment a map of full crystal orientations into a grain-ID image on the device (ggnn_label_orientations; include/ggnn.h
    states the rule, tests/orientcheck.py restates it): `label_grains` with the link decided by the DISORIENTATION of
    two neighbours under crystal symmetry, and a symmetry-aware mean orientation per grain.

    quats: float32 [4, ny, nx] on the device (w, x, y, z planes; crystal to sample; q and -q are one orientation;
    `quaternions_from_bunge` makes them from Euler angles); a pixel is valid when | |q|^2 - 1 | <= 1e-3 (NaN: non-indexed) and
    the optional mask `valid` allows it.  tol: two 4-neighbours are linked when their disorientation angle is at most tol
    (radians, in (0, pi/2); fp32 resolves about 1e-5 rad at 1 degree).  symmetry: "cubic" (the 24 proper rotations: the indexing
    software may report any equivalent at any pixel) or "none".  min_pixels, max_sweeps, boundary, grain_capacity: as in
    `label_grains`.

    -> (image int32 [ny, nx], n_grain, mean_quats float32 [4, n_grain], status dict) as `label_grains` gives them; a grain's
    mean runs over the pixels of its original component, each aligned to the equivalent nearest the component's first pixel,
    and is normalised (no-flux: row 0, the boundary grain's, is the identity); `growth_angles` turns it into theta_x and theta_z.
    Device tensors in, device tensors out, ONE read-back (the status); 12 + 2 max_sweeps launches whatever the map holds.

    A stack of equal-shaped maps in the same launches is `label_orientation_maps`.  Not covered: hexagonal and other groups,
    8-connectivity.  A component whose pixels drift more
    than about 20 degrees from its first pixel can align a pixel to the wrong equivalent."""
    v = _label_orient(quats, tol, valid, min_pixels, max_sweeps, boundary, grain_capacity, symmetry)
    status = dict(zip(LABEL_STATUS_WORDS, v["status"].tolist()))   # the one read-back
    if status["n_bound_hits"]:
        raise _lib.GGNNError(f"ggnn_label_orientations: {status['n_bound_hits']} threads reached the bound of a parent walk: {status}")
    n_grain = status["n_grains"] + (1 if boundary == "noflux" else 0)
    return v["image"], n_grain, v["means"][:, :min(n_grain, v["capacity"])].contiguous(), status


def sample_from_euler_map(phi1, Phi, phi2, G, R, tol, min_pixels=1, degrees=False, **kw):
    """A rollout's first state from an EBSD map: `quaternions_from_bunge` on the three Euler-angle maps ([ny, nx]),
    `label_orientations` (tol in radians; symmetry, valid, max_sweeps and grain_capacity go to it), `growth_angles` of the mean
    orientations read back, and `sample_from_image` on the labelled image with everything it takes (span, patch_pixels, grid,
    merge_radius, boundary, links, ...).

    -> (x_dict, edge_index_dict, edge_attr, image, status): the first three are bit for bit what
    `sample_from_image(image, theta_x, theta_z, ...)` gives on the returned image and the float32 growth angles; status is the
    labelling's, with "mean_quats" (device float32 [4, n_grain]), "theta_x" and "theta_z" (host float32)."""
    boundary = kw.get("boundary", "periodic")
    label_kw = {k: kw.pop(k) for k in ("valid", "max_sweeps", "grain_capacity", "symmetry") if k in kw}
    quats = quaternions_from_bunge(phi1, Phi, phi2, degrees)
    quats = quats if quats.is_cuda else quats.cuda()
    if quats.dim() != 3:
        raise _lib.GGNNError("phi1, Phi and phi2 must be [ny, nx] maps")
    image, n_grain, means, status = label_orientations(quats, tol, min_pixels=min_pixels, boundary=boundary, **label_kw)
    if status["overflow"]:
        raise ValueError(f"the map has more grains than grain_capacity: {status}")
    theta_x, theta_z = (t.cpu().numpy().astype(np.float32) for t in growth_angles(means))
    x, ei, ea = sample_from_image(image, theta_x, theta_z, G, R, n_grain=n_grain, **kw)
    return x, ei, ea, image, dict(status, mean_quats=means, theta_x=theta_x, theta_z=theta_z)


def samples_from_euler_maps(phi1, Phi, phi2, G, R, tol, min_pixels=1, degrees=False, **kw):
    """A union rollout's first state from a stack of EBSD maps: `quaternions_from_bunge` on the three stacks of Euler angles
    ([T, ny, nx]), `label_orientation_maps` (tol in radians; symmetry, valid, max_sweeps and grain_capacity go to it),
    `growth_angles` of the mean orientations read back once, and `samples_from_images` on the labelled images with
    everything it takes (G and R: scalars or one value per map).

    -> (x_dict, edge_index_dict, edge_attr, traj_offsets, images, statuses) as `samples_from_orientation_maps` gives them:
    every trajectory's rows are, bit for bit, `sample_from_euler_map`'s on that map alone; every status also holds "mean_quats"
    (device float32 [4, n_grain]).  Three read-backs whatever T.  A map that overflows grain_capacity raises and is named."""
    label_kw = {k: kw.pop(k) for k in ("valid", "max_sweeps", "grain_capacity", "symmetry") if k in kw}
    quats = quaternions_from_bunge(phi1, Phi, phi2, degrees)
    quats = quats if quats.is_cuda else quats.cuda()
    if quats.dim() != 4:
        raise _lib.GGNNError("phi1, Phi and phi2 must be [T, ny, nx] stacks of maps")
    images, n_grains, means, statuses = label_orientation_maps(quats, tol, min_pixels=min_pixels, boundary=kw.get("boundary", "periodic"),
                                                               **label_kw)
    _no_map_overflows(statuses)
    host = means[:, :, :max(n_grains)].cpu().numpy()                       # every map's rows in one read-back
    theta = [tuple(a.astype(np.float32) for a in growth_angles(host[t, :, :n])) for t, n in enumerate(n_grains)]
    statuses = [dict(s, mean_quats=means[t, :, :n].contiguous()) for t, (s, n) in enumerate(zip(statuses, n_grains))]
    return _union_from_labelled(images, n_grains, statuses, theta, G, R, kw)


# ---- ids that persist across a sequence of labelled maps --------------------------------------------------------------------

LINK_FRAME_WORDS = ("n_local", "n_matched", "n_fresh", "n_split", "n_gone", "n_vote_overflow")
LINK_MAX_DEFAULT_CAPACITY = 65536   # the default room per frame: a frame's slot table takes 128 bytes a row


def _link(labels, n_local, means, match_tol, min_overlap, boundary, local_capacity, global_capacity):
    """Every launch of `link_labels`, no read-back: -> dict of the relabelled frames, gid, pred, first_frame, last_frame, theta
    (None without means), the status words on the device, and the call's arguments with what they point to
    (tools/vectorize_cost.py).  labels int32 [T, ny, nx], n_local int64 [T], means float32 [T, K, local_capacity] or None: all
    contiguous, on one device."""
    be = default_backend()
    T, ny, nx = labels.shape
    K, dev = (0 if means is None else means.size(1)), labels.device
    frames = torch.empty_like(labels)
    gid = torch.empty(T, local_capacity, dtype=torch.int32, device=dev)
    pred = torch.empty(T, local_capacity, dtype=torch.int32, device=dev)
    first_frame = torch.empty(global_capacity, dtype=torch.int32, device=dev)
    last_frame = torch.empty(global_capacity, dtype=torch.int32, device=dev)
    theta = torch.empty(K, global_capacity, dtype=torch.float32, device=dev) if K else None
    status = torch.empty(_lib.GGNN_LINK_FRAME_WORDS * T + _lib.GGNN_LINK_GLOBAL_WORDS, dtype=torch.int64, device=dev)   # (zeroed by the call)
    need = be.lib.ggnn_link_workspace_bytes(T, local_capacity, K)
    if need == 0:
        raise _lib.GGNNError(f"ggnn_link_labels takes no stack of {T} frames with room for {local_capacity} grains each")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    A = _lib.LinkLabelsArgs()
    A.labels, A.n_local, A.means, A.frames_out, A.gid, A.pred = (_lib.ptr(labels), _lib.ptr(n_local), _lib.ptr(means), _lib.ptr(frames),
                                                                  _lib.ptr(gid), _lib.ptr(pred))
    A.first_frame, A.last_frame, A.theta, A.status = _lib.ptr(first_frame), _lib.ptr(last_frame), _lib.ptr(theta), _lib.ptr(status)
    A.workspace, A.workspace_bytes = _lib.ptr(ws), need
    A.T, A.nx, A.ny, A.local_capacity, A.global_capacity, A.min_overlap = T, nx, ny, local_capacity, global_capacity, min_overlap
    A.match_tol, A.use_match_tol = (0.0 if match_tol is None else float(np.float32(match_tol))), int(match_tol is not None)
    A.K, A.boundary = K, BOUNDARIES[boundary]
    _lib.check(be.lib.ggnn_link_labels(ctypes.byref(A), _lib.current_stream()), "ggnn_link_labels")
    return {"frames": frames, "gid": gid, "pred": pred, "first_frame": first_frame, "last_frame": last_frame, "theta": theta,
            "status": status, "boundary": boundary, "calls": (A, labels, n_local, means, ws)}


def _link_checked(labels, n_local, means, match_tol, min_overlap, boundary, local_capacity, global_capacity):
    """`_link` behind the checks that `link_labels` and `label_sequence` share: -> its dict."""
    _check_boundary(boundary)
    labels = _image_tensor(labels, 3, "labels must be a [T, ny, nx] device tensor of labelled frames", "labels")
    T, ny, nx = labels.shape
    if T < 1 or nx < 3 or ny < 3:
        raise _lib.GGNNError("labels must hold at least one frame of at least 3 x 3 pixels")
    if isinstance(n_local, torch.Tensor):
        if not n_local.is_cuda or n_local.numel() != T:
            raise _lib.GGNNError("n_local must be a device tensor or a host list of one count per frame")
        n_local = n_local.reshape(-1).to(torch.int64).contiguous()
        most = None
    else:
        host = [int(n) for n in n_local]
        if len(host) != T:
            raise _lib.GGNNError("n_local must be a device tensor or a host list of one count per frame")
        most = max(max(host), 1)
        n_local = torch.tensor(host, dtype=torch.int64, device=labels.device)
    if means is not None:
        if not isinstance(means, torch.Tensor) or not means.is_cuda or means.dim() != 3 or means.size(0) != T or means.dtype != torch.float32:
            raise _lib.GGNNError("means must be a float32 [T, K, local_capacity] device tensor")
        if not 0 <= means.size(1) <= 4:
            raise _lib.GGNNError("means must hold at most 4 channels")
        if local_capacity is not None and int(local_capacity) != means.size(2):
            raise _lib.GGNNError("local_capacity must be the row length of means")
        local_capacity = means.size(2)
        means = means.contiguous() if means.size(1) else None
    if match_tol is not None and (means is None or not float(match_tol) >= 0):
        raise _lib.GGNNError("match_tol needs means and must be >= 0")
    if int(min_overlap) < 1:
        raise _lib.GGNNError("min_overlap must be at least 1")
    if local_capacity is None:
        local_capacity = most if most is not None else min(ny * nx, LINK_MAX_DEFAULT_CAPACITY)
    local_capacity = int(local_capacity)
    global_capacity = local_capacity * min(T, 2) if global_capacity is None else int(global_capacity)
    if local_capacity < 1 or global_capacity < 1:
        raise _lib.GGNNError("local_capacity and global_capacity must be at least 1")
    return _link(labels, n_local, means, match_tol, int(min_overlap), boundary, local_capacity, global_capacity)


def _link_report(v, words):
    """The status words of a link call as the report of `link_labels`, and its results cut to what the sequence holds; raises on
    a dropped vote and on an overflow."""
    T = v["frames"].size(0)
    W = _lib.GGNN_LINK_FRAME_WORDS
    per_frame = [dict(zip(LINK_FRAME_WORDS, words[W * t:W * t + W])) for t in range(T)]
    n_global, overflow = words[W * T], words[W * T + 1]
    dropped = sum(s["n_vote_overflow"] for s in per_frame)
    if dropped:
        raise _lib.GGNNError(f"ggnn_link_labels: {dropped} votes found the {_lib.GGNN_LINK_SLOTS} slots of their grain taken (a grain "
                             f"overlaps more grains of the frame before: the frames are too far apart): {per_frame}")
    if overflow:
        raise _lib.GGNNError(f"ggnn_link_labels: overflow {overflow} (ids beyond the local capacity, or {n_global} global grains "
                             f"beyond the global capacity {v['first_frame'].numel()}): {per_frame}")
    noflux = v["boundary"] == "noflux"
    n_grain = n_global + (1 if noflux else 0)
    theta = v["theta"]
    if theta is not None:
        theta = theta[:, :n_global]
        if noflux:                                         # row 0: the boundary grain's, as label_grains writes it
            theta = torch.cat([torch.zeros(theta.size(0), 1, dtype=theta.dtype, device=theta.device), theta], 1)
        theta = theta.contiguous()
    report = {"frames": per_frame, "n_global": n_global, "gid": v["gid"], "pred": v["pred"],
              "first_frame": v["first_frame"][:n_global].contiguous(), "last_frame": v["last_frame"][:n_global].contiguous()}
    return v["frames"], n_grain, theta, report


def link_labels(labels, n_local, means=None, match_tol=None, min_overlap=1, boundary="periodic", local_capacity=None,
                global_capacity=None):
    """Give the grains of a stack of labelled frames ids that persist from frame to frame, on the device (ggnn_link_labels;
    include/ggnn.h states the rule, tests/linkcheck.py restates it): the grains of consecutive frames are linked by
    their pixel overlap and the whole stack is renumbered, which is what `frames_to_samples` needs and what labelling each frame
    on its own does not give.

    labels: integer [T, ny, nx] on the device, every frame labelled on its own whatever its numbering, as `label_grains` writes
    it: local ids first .. first + n_local[t] - 1, first = 1 ("periodic") or 2 ("noflux": id 1 is the boundary grain and stays 1),
    0 = unfilled (it never votes and stays 0).  n_local: a device tensor or a host list of T counts.  means: float32
    [T, K, local_capacity] on the device, 0 <= K <= 4, row b - first of frame t the mean of local grain b; with match_tol the
    predecessor must also lie within match_tol of the grain in every channel (one fp32 subtraction each).  min_overlap: the
    fewest shared pixels that make a candidate.  local_capacity: rows per frame (default: the row length of means, the largest
    of a host n_local, else min(ny nx, 65536)); global_capacity: rows of the per-grain results (default min(T, 2)
    local_capacity).

    The rule: a grain's predecessor is the grain of the frame before that shares the most pixels with it (a tie: the smaller
    id); when several grains claim one predecessor the one that shares the most keeps it (a tie: the smaller id) and the others
    are FRESH; frame 0 keeps its ids, fresh grains are numbered after them by frame and then by local id.  A grain pinched in two
    keeps its id on the larger part.  A grain that is absent from one frame and present in the next comes back fresh.

    -> (frames int32 [T, ny, nx], n_grain, theta float32 [K, n_grain] or None, report): theta is every grain's mean in its first
    frame (no-flux: row 0, the boundary grain's, is 0); report = {"frames": per frame a dict of n_local, n_matched, n_fresh,
    n_split, n_gone, n_vote_overflow; "n_global"; "gid", "pred": int32 [T, local_capacity] device tensors, row b - first;
    "first_frame", "last_frame": int32 [n_global] device tensors, row g - first}.  Device tensors in, device tensors out, ONE
    read-back (the status); five launches whatever T and whatever the frames hold.  Raises when a vote was dropped (a grain that
    overlaps more than 16 grains of the frame before) and on an overflow of either capacity."""
    v = _link_checked(labels, n_local, means, match_tol, min_overlap, boundary, local_capacity, global_capacity)
    return _link_report(v, v["status"].tolist())           # the one read-back


def label_sequence(ids=None, angles=None, tol=None, valid=None, min_pixels=1, max_sweeps=64, boundary="periodic", match_tol=None,
                   min_overlap=1, grain_capacity=None):
    """A sequence of measured maps -- in-situ EBSD, serial sections, a phase-field run exported as orientations -- into grain-ID
    images whose ids persist: ONE stacked labelling call (`label_maps`' launches) on the current stream, then `link_labels`' on
    the stack, with nothing read back in between (every frame's number of grains goes from the labelling's status to the linking on the
    device) and ONE read-back at the end, of the T label status rows and the link status together.

    Exactly one of ids -- integer [T, ny, nx] -- and angles -- float32 [T, K, ny, nx] with tol --, on the device; valid: an
    optional [T, ny, nx] mask; min_pixels, max_sweeps, boundary: as in `label_grains`; match_tol (angles only), min_overlap: as in
    `link_labels`, the means being the labelling's.  grain_capacity: room per frame (default min(ny nx // min_pixels + 2, 65536)).

    -> (frames, n_grain, theta, report) as `link_labels` gives them; report["label"] is the per-frame `label_grains` status.
    Raises on n_bound_hits, as `label_grains` does, and on an overflow of a frame's labelling.  Neither the labelling launches
    nor the linking launches grow with T."""
    _check_boundary(boundary)
    if (ids is None) == (angles is None):
        raise _lib.GGNNError("exactly one of ids and angles must be given")
    src = ids if angles is None else angles
    if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dim() != (3 if angles is None else 4) or src.size(0) < 1:
        raise _lib.GGNNError("ids must be a [T, ny, nx], angles a [T, K, ny, nx] device tensor")
    T, (ny, nx) = src.size(0), src.shape[-2:]
    if valid is not None and (not isinstance(valid, torch.Tensor) or valid.shape != (T, ny, nx)):
        raise _lib.GGNNError("valid must be a [T, ny, nx] device mask")
    noflux = boundary == "noflux"
    cap = min(ny * nx // max(int(min_pixels), 1) + 2, LINK_MAX_DEFAULT_CAPACITY) if grain_capacity is None else int(grain_capacity)
    if cap < (2 if noflux else 1):
        raise _lib.GGNNError("grain_capacity must hold at least one grain")
    stacked = _label_stack(ids, angles, tol, valid, min_pixels, max_sweeps, boundary, cap)
    return _link_frames(stacked, match_tol, min_overlap, boundary, cap, "ggnn_label_grains_stack")


def _link_frames(stacked, match_tol, min_overlap, boundary, cap, entry):
    """The frames of a sequence, labelled as a stack by `entry` (the dict of `_label_stack` or `_label_orient_stack`), linked on
    the device, and the ONE read-back of both statuses -> what `label_sequence` returns."""
    labels, label_status, means = stacked["image"], stacked["status"], stacked["means"]
    T, noflux = labels.size(0), boundary == "noflux"
    n_local = label_status[:, LABEL_STATUS_WORDS.index("n_grains")].contiguous()
    if means is not None and noflux:                       # (row 0 is the boundary grain's: local grain b is row b - 2 from here on)
        means = means[:, :, 1:].contiguous()
    v = _link_checked(labels, n_local, means, match_tol, min_overlap, boundary, cap - 1 if noflux else cap, None)
    words = torch.cat([label_status.reshape(-1), v["status"]]).tolist()   # the one read-back
    n = len(LABEL_STATUS_WORDS)
    _, label_report = _stack_statuses(stacked, words[:n * T], entry)
    for t, s in enumerate(label_report):
        if s["overflow"]:
            raise _lib.GGNNError(f"frame {t} has more grains than grain_capacity {cap}: {s}")
    frames, n_grain, theta, report = _link_report(v, words[n * T:])
    report["label"] = label_report
    return frames, n_grain, theta, report


def samples_from_orientation_sequence(theta_x_maps, theta_z_maps, G, R, tol, min_pixels=1, **kw):
    """A training set from a recorded sequence of orientation maps: `label_sequence` on the two stacks of angle maps
    ([T, ny, nx] float32 on the device, radians), the per-grain angles of every grain's first frame read back, and
    `frames_to_samples` on the relabelled frames with everything it takes (span, patch_pixels, extra_volume, z, grid,
    merge_radius, joint_capacity, boundary, links, max_trace); valid, max_sweeps, match_tol, min_overlap and grain_capacity go to
    `label_sequence`.

    -> (samples, report, frames): samples and report as `frames_to_samples` gives them on the returned frames; report["sequence"]
    is `label_sequence`'s report, with the angles under "theta_x" and "theta_z" (host float32)."""
    if (not isinstance(theta_x_maps, torch.Tensor) or not isinstance(theta_z_maps, torch.Tensor) or theta_x_maps.dim() != 3
            or theta_x_maps.shape != theta_z_maps.shape):
        raise _lib.GGNNError("theta_x_maps and theta_z_maps must be equal-shaped [T, ny, nx] device tensors")
    seq_kw = {k: kw.pop(k) for k in ("valid", "max_sweeps", "match_tol", "min_overlap", "grain_capacity") if k in kw}
    angles = torch.stack([theta_x_maps.to(torch.float32), theta_z_maps.to(torch.float32)], 1)
    frames, n_grain, theta, sequence = label_sequence(angles=angles, tol=tol, min_pixels=min_pixels, boundary=kw.get("boundary", "periodic"),
                                                      **seq_kw)
    angles_host = theta.cpu().numpy()
    samples, report = frames_to_samples(frames, angles_host[0], angles_host[1], G, R, **kw)
    report["sequence"] = dict(sequence, theta_x=angles_host[0], theta_z=angles_host[1])
    return samples, report, frames


def label_orientation_sequence(quats, tol, valid=None, min_pixels=1, max_sweeps=64, boundary="periodic", match_tol=None,
                               min_overlap=1, grain_capacity=None, symmetry="cubic"):
    """`label_sequence` for maps of full orientations: ONE stacked labelling call (`label_orientation_maps`' launches) on quats
    (float32 [T, 4, ny, nx] on the device), then `link_labels`' on the stack by pixel overlap alone, with ONE read-back at the
    end.

    -> (frames, n_grain, quat float32 [4, n_grain], report) as `label_sequence` gives them: quat is every grain's mean
    orientation in its first frame, copied (no-flux: row 0 is the identity).  match_tol raises: a per-channel gate on quaternion
    components means nothing (a grain's mean may land on another equivalent in the next frame); a symmetry-aware gate is not
    covered."""
    _check_boundary(boundary)
    if match_tol is not None:
        raise _lib.GGNNError("match_tol is a per-channel gate and means nothing on quaternion components: frames of orientations "
                             "are linked by overlap alone")
    if not isinstance(quats, torch.Tensor) or not quats.is_cuda or quats.dim() != 4 or quats.size(0) < 1:
        raise _lib.GGNNError("quats must be a float32 [T, 4, ny, nx] device tensor")
    T, (ny, nx) = quats.size(0), quats.shape[-2:]
    if valid is not None and (not isinstance(valid, torch.Tensor) or valid.shape != (T, ny, nx)):
        raise _lib.GGNNError("valid must be a [T, ny, nx] device mask")
    noflux = boundary == "noflux"
    cap = min(ny * nx // max(int(min_pixels), 1) + 2, LINK_MAX_DEFAULT_CAPACITY) if grain_capacity is None else int(grain_capacity)
    if cap < (2 if noflux else 1):
        raise _lib.GGNNError("grain_capacity must hold at least one grain")
    stacked = _label_orient_stack(quats, tol, valid, min_pixels, max_sweeps, boundary, cap, symmetry)
    frames, n_grain, quat, report = _link_frames(stacked, None, min_overlap, boundary, cap, "ggnn_label_orientations_stack")
    if noflux:
        quat[0, 0] = 1.0                                   # the boundary grain's row, as label_orientations writes it
    return frames, n_grain, quat, report


def samples_from_euler_sequence(phi1, Phi, phi2, G, R, tol, min_pixels=1, degrees=False, **kw):
    """A training set from a recorded sequence of EBSD maps: `quaternions_from_bunge` on the three stacks of Euler angles
    ([T, ny, nx]), `label_orientation_sequence`, `growth_angles` of every grain's orientation in its first frame, and
    `frames_to_samples` on the relabelled frames with everything it takes; valid, max_sweeps, min_overlap, grain_capacity and
    symmetry go to `label_orientation_sequence`.

    -> (samples, report, frames): samples and report as `frames_to_samples` gives them on the returned frames; report["sequence"]
    is `label_orientation_sequence`'s report, with "quat" (device float32 [4, n_grain]), "theta_x" and "theta_z" (host float32)."""
    seq_kw = {k: kw.pop(k) for k in ("valid", "max_sweeps", "match_tol", "min_overlap", "grain_capacity", "symmetry") if k in kw}
    quats = quaternions_from_bunge(phi1, Phi, phi2, degrees)
    quats = quats if quats.is_cuda else quats.cuda()
    if quats.dim() != 4:
        raise _lib.GGNNError("phi1, Phi and phi2 must be [T, ny, nx] stacks of maps")
    frames, n_grain, quat, sequence = label_orientation_sequence(quats, tol, min_pixels=min_pixels, boundary=kw.get("boundary", "periodic"),
                                                                 **seq_kw)
    theta_x, theta_z = (t.cpu().numpy().astype(np.float32) for t in growth_angles(quat))
    samples, report = frames_to_samples(frames, theta_x, theta_z, G, R, **kw)
    report["sequence"] = dict(sequence, quat=quat, theta_x=theta_x, theta_z=theta_z)
    return samples, report, frames
