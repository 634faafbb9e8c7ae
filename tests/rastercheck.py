"""The grain-ID image of a layer's grain polygons, restated in numpy: the definition ggnn_polygons_rasterize
(csrc/raster.hip, include/ggnn.h) is held to bit for bit, and what the reference's plot_polygons (graph_datastruct.py:553-610)
draws through PIL up to PIL's own choices on polygon boundaries (tests/test_grain_image.py).

The rule, exact in integers:
  vertex pixels  v = (int)(x * (float)s) for a periodic layer (one float32 product, truncated toward zero: the reference's
                 np.asarray(coor * s, dtype=int)), v = (int)rint(x * (float)s) for a no-flux one (half to even: np.round), both
                 coordinates scaled by s = size[0]; the product saturates at +-2^20 (NaN: -2^20), far outside any canvas
  membership     a lattice point belongs to a polygon when it lies on one of its edges or has an odd number of crossings
                 under the half-open rule in y -- edge (a, b) with ya < yb counts for ya <= y < yb when the point is strictly
                 left of it -- decided by signs of int64 cross products: the closed set of the even-odd rule
  ownership      the highest grain index + 1 among the polygons that contain the point; 0 = uncovered
  periodic       canvas [0, 2s)^2, points outside dropped, folded to [0, s)^2 by mod s with max
  no-flux        canvas size[0] x size[1], the boundary grain of every trajectory skipped, uncovered pixels filled from
                 corner_grains[2x // nx + 2 (2y // ny)] when corner_grains is given
Membership is decided by brute force: every lattice point of a polygon's clipped bounding box against every edge."""
import numpy as np

SATURATE = float(2 ** 20)


def vertex_pixels(xy, s, boundary):
    """int64 [n, 2] from fp32 [n, 2]."""
    p = np.asarray(xy, np.float32).reshape(-1, 2) * np.float32(s)      # one float32 product per coordinate
    if boundary == "noflux":
        p = np.rint(p)
    with np.errstate(invalid="ignore"):
        p = np.fmin(np.fmax(p, np.float32(-SATURATE)), np.float32(SATURATE))   # (fmax / fmin: NaN -> the bound)
    return np.trunc(p).astype(np.int64)


def contains(v, px, py):
    """Closed even-odd membership of the lattice points (px, py) (int64 arrays of one shape) in the integer polygon v."""
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    odd, on = np.zeros(px.shape, bool), np.zeros(px.shape, bool)
    n = len(v)
    if n < 2:
        return on
    for i in range(n):
        (x0, y0), (x1, y1) = v[i], v[(i + 1) % n]
        cross = (px - x0) * (y1 - y0) - (py - y0) * (x1 - x0)
        on |= (cross == 0) & (px >= min(x0, x1)) & (px <= max(x0, x1)) & (py >= min(y0, y1)) & (py <= max(y0, y1))
        if y0 != y1:
            if y0 > y1:                       # (a, b) with ya < yb: the cross product changes sign with the direction
                cross, y0, y1 = -cross, y1, y0
            odd ^= (py >= y0) & (py < y1) & (cross < 0)   # strictly left of the edge: (px - xa) dy < (py - ya) dx
    return odd | on


def polygon_points(v, width, height):
    """(ys, xs) of the lattice points of [0, width) x [0, height) that belong to the integer polygon v."""
    if len(v) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    x0, x1 = max(int(v[:, 0].min()), 0), min(int(v[:, 0].max()), width - 1)
    y0, y1 = max(int(v[:, 1].min()), 0), min(int(v[:, 1].max()), height - 1)
    if x0 > x1 or y0 > y1:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    py, px = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
    inside = contains(v, px, py)
    return py[inside], px[inside]


def boundary_grains(n_grain, boundary, traj_grain_off=None):
    """The grains a no-flux image skips: grain 0, or the first grain of every trajectory that has grains."""
    if boundary != "noflux":
        return set()
    if traj_grain_off is None:
        return {0}
    off = [int(o) for o in traj_grain_off]
    return {a for a, b in zip(off[:-1], off[1:]) if b > a}


def grain_image(rowptr, xy_sorted, size, boundary="periodic", traj_grain_off=None, grains=None, corner_grains=None):
    """int32 [ny, nx] (periodic: [s, s]) of one layer.  rowptr / xy_sorted: the layer's arena row (rowptr of the WHOLE layer);
    grains = (g0, g1): only that range, with ids counted from g0 (a trajectory's slice)."""
    rowptr, xy = np.asarray(rowptr, np.int64), np.asarray(xy_sorted, np.float32).reshape(-1, 2)
    nx, ny = int(size[0]), int(size[1])
    s = nx
    n_grain = len(rowptr) - 1
    g0, g1 = (0, n_grain) if grains is None else (int(grains[0]), int(grains[1]))
    skip = boundary_grains(n_grain, boundary, traj_grain_off)
    periodic = boundary == "periodic"
    width, height = (2 * s, 2 * s) if periodic else (nx, ny)
    img = np.zeros((s, s) if periodic else (ny, nx), np.int32)
    for g in range(g0, g1):
        if g in skip or rowptr[g + 1] - rowptr[g] < 2:
            continue
        ys, xs = polygon_points(vertex_pixels(xy[rowptr[g]:rowptr[g + 1]], s, boundary), width, height)
        if periodic:
            ys, xs = ys % s, xs % s
        np.maximum.at(img, (ys, xs), np.int32(g - g0 + 1))
    if not periodic and corner_grains is not None:
        x, y = np.meshgrid(np.arange(nx), np.arange(ny))
        patch = 2 * x // nx + 2 * (2 * y // ny)
        img = np.where(img == 0, np.asarray(corner_grains, np.int32)[patch], img).astype(np.int32)
    return img


def compare(image, truth, n_grain):
    """(differing pixels, per-id counts int64 [n_grain + 1]; ids outside 0..n_grain are not counted)."""
    image = np.asarray(image)
    ids = image[(image >= 0) & (image <= n_grain)]
    counts = np.bincount(ids.ravel(), minlength=n_grain + 1).astype(np.int64)
    return (None if truth is None else int((image != np.asarray(truth)).sum())), counts
