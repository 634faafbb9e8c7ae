"""Linking junctions by tracing boundaries (ggnn_image_junction_windows_traj / ggnn_junction_links_trace_traj, include/ggnn.h;
vectorize's links="trace"), restated in numpy on top of tests/vectorcheck.py, tests/vectorcheck_noflux.py and
tests/vectorcheck_union.py: the definition the kernel is held to bit for bit.

The present rule links junction j = {a, b, c} for its pair (a, b) to the ONE other junction whose triple holds both grains and
leaves the column at -1 (an OPEN pair) when there is none or more than one.  More than one is what two grains look like that
share two separate stretches of boundary: a lens on a boundary, a band from wall to wall.  This rule touches the open columns
only, per image, and follows the a | b boundary through the image from j to the junction at its other end.  Exact in integers.

  vertex     a window (y, x) of the junction rule: the same range, the same periodic wrap, the same outside-reads-as-id-1
             convention of a no-flux image (an inside pixel that is 1 or outside [1, n_grain] reads as 0 there)
  cracks     a vertex has four: UP between TL and TR to (y - 1, x), DOWN between BL and BR to (y + 1, x), LEFT between TL and BL
             to (y, x - 1), RIGHT between TR and BR to (y, x + 1); a crack is an a | b crack when its two pixels are the ids
             of grains a and b
  rep        rep[j] = the raster index of junction j's representative window within its image
  owner      a window W that carries key k is owned by the junction of smallest index among the kept ones (j <
             min(n_joint, joint_capacity)) that has triple k and whose representative lies at an offset within merge_radius of
             W (wrapped for periodic, plain for no-flux); a carrier that no junction owns belongs to nobody (chain merges)
  owned by j the windows at offsets within merge_radius of rep[j] that carry j's triple and whose owner for it is j
  exits      for j and its pair (a, b): the a | b cracks from a vertex owned by j to a vertex not owned by j, in the order of
             the offsets (dy, then dx, then UP, DOWN, LEFT, RIGHT)
  diagonals  for j and (a, b): the quadruple windows owned by j whose (TL, BR) are a and b
  walk       j has no diagonal and exactly one exit: follow it.  At every vertex reached: if the window carries a key that
             holds both a and b, stop -- the owner of that carrier is o; otherwise the vertex must have exactly two a | b cracks,
             the one arrived by and one more: leave by the other.  The walk FAILS at a vertex with another number of a | b
             cracks (four: the two-id checkerboard window [a b; b a]), at a carrier nobody owns, and OVERFLOWS when more than
             max_trace vertices would be reached (default 4 (nx + ny))
  accept     partner(j, pair) = o only if o too has no diagonal and exactly one exit for (a, b): that exit is the crack arrived
             by, so partner(o, pair) = j by the reversed walk, of the same length
  quadruple  j has exactly one diagonal W for (a, b): o = the owner of W's other key; partner(j, pair) = o when o too has
             exactly one diagonal for (a, b), and it is W.  There is no crack to follow.  More than one diagonal fails.
  counters   n_traced, n_trace_failed (no or several exits, a failed walk, a refused partner), n_trace_overflow: directed
             columns, per image; every open column is counted in exactly one.  n_open_pairs of the status becomes what is
             still open, n_open_pairs - n_traced.
Owners are found in a dict of triples, windows by brute force."""
import numpy as np

import vectorcheck as vc
import vectorcheck_noflux as vn
import vectorcheck_union as vu
from vectorcheck import PAIRS, window_keys

COUNTERS = ("n_traced", "n_trace_failed", "n_trace_overflow")
STEP = ((-1, 0), (1, 0), (0, -1), (0, 1))       # UP, DOWN, LEFT, RIGHT
OPPOSITE = (1, 0, 3, 2)


def default_max_trace(ny, nx):
    return 4 * (nx + ny)


class Windows:
    """The vertex conventions of one image."""

    def __init__(self, image, n_grain, merge_radius, boundary):
        img = np.asarray(image).astype(np.int64)
        self.ny, self.nx = img.shape
        self.n_grain, self.R, self.periodic = int(n_grain), int(merge_radius), boundary == "periodic"
        assert boundary in ("periodic", "noflux")
        if self.periodic:
            self.img = img
        else:
            pad = np.ones((self.ny + 2, self.nx + 2), np.int64)
            pad[1:-1, 1:-1] = np.where((img < 2) | (img > n_grain), 0, img)
            self.img = pad

    def pixel(self, y, x):
        if self.periodic:
            return int(self.img[y % self.ny, x % self.nx])
        if -1 <= y <= self.ny and -1 <= x <= self.nx:
            return int(self.img[y + 1, x + 1])
        return 1

    def in_range(self, y, x):
        return self.periodic or (-1 <= y < self.ny and -1 <= x < self.nx)

    def norm(self, y, x):
        return (y % self.ny, x % self.nx) if self.periodic else (y, x)

    def raster(self, y, x):
        return y * self.nx + x if self.periodic else (y + 1) * (self.nx + 1) + (x + 1)

    def window(self, r):
        if self.periodic:
            return divmod(int(r), self.nx)
        y, x = divmod(int(r), self.nx + 1)
        return y - 1, x - 1

    def pixels(self, y, x):
        return self.pixel(y, x), self.pixel(y, x + 1), self.pixel(y + 1, x), self.pixel(y + 1, x + 1)

    def keys(self, y, x):
        return window_keys(*self.pixels(y, x), self.n_grain)[0]

    def near(self, ya, xa, yb, xb):
        """Is (yb, xb) at an offset within R of (ya, xa)."""
        if self.periodic:
            dy, dx = (yb - ya) % self.ny, (xb - xa) % self.nx
            return (dy <= self.R or dy >= self.ny - self.R) and (dx <= self.R or dx >= self.nx - self.R)
        return abs(yb - ya) <= self.R and abs(xb - xa) <= self.R

    def cracks(self, y, x):
        tl, tr, bl, br = self.pixels(y, x)
        return (tl, tr), (bl, br), (tl, bl), (tr, br)

    def representatives(self):
        """[(raster index, key)] of every junction, in the order of the numbering."""
        if self.periodic:
            tl, tr = self.img, np.roll(self.img, -1, 1)
            bl, br = np.roll(self.img, -1, 0), np.roll(np.roll(self.img, -1, 0), -1, 1)
            first = 0
        else:
            tl, tr, bl, br = self.img[:-1, :-1], self.img[:-1, 1:], self.img[1:, :-1], self.img[1:, 1:]
            first = -1
        stack = np.sort(np.stack([tl, tr, bl, br]), axis=0)
        distinct = 1 + (stack[1:] != stack[:-1]).sum(0)
        carriers = {}
        for i, k in zip(*np.nonzero(distinct >= 3)):
            y, x = int(i) + first, int(k) + first
            for key in self.keys(y, x):
                carriers.setdefault(key, []).append((y, x))
        out = []
        for key, ws in carriers.items():
            for (y, x) in ws:
                if not any(self.near(y, x, y2, x2) and self.raster(y2, x2) < self.raster(y, x) for (y2, x2) in ws):
                    out.append((self.raster(y, x), key))
        return sorted(out)


class Tracer:
    """The rule on one image: W its Windows, triples [n, 3] local, rep [n]."""

    def __init__(self, W, triples, rep):
        self.W, self.rep = W, rep
        self.keys = [tuple(int(g) for g in t) for t in triples]
        self.by_key = {}
        for j, k in enumerate(self.keys):
            self.by_key.setdefault(k, []).append(j)

    def owner(self, y, x, key):
        for o in self.by_key.get(key, []):
            if self.W.near(*self.W.window(self.rep[o]), y, x):
                return o
        return None

    def owned(self, j, y, x):
        W = self.W
        return W.in_range(y, x) and self.keys[j] in W.keys(y, x) and self.owner(y, x, self.keys[j]) == j

    def exits(self, j, a, b):
        """-> ([(vertex reached y, x, crack taken)], [the diagonals (y, x)]) of junction j for the grains a, b."""
        W, R = self.W, self.W.R
        want = {a + 1, b + 1}
        ry, rx = W.window(self.rep[j])
        found, diagonals = [], []
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                if not W.in_range(ry + dy, rx + dx):
                    continue
                y, x = W.norm(ry + dy, rx + dx)
                if not self.owned(j, y, x):
                    continue
                tl, _, _, br = W.pixels(y, x)
                if len(W.keys(y, x)) == 2 and {tl, br} == want:
                    diagonals.append((y, x))
                for d, crack in enumerate(W.cracks(y, x)):
                    if set(crack) == want:
                        y2, x2 = W.norm(y + STEP[d][0], x + STEP[d][1])
                        if not self.owned(j, y2, x2):
                            found.append((y2, x2, d))
        return found, diagonals

    def partner(self, j, a, b, max_trace):
        """-> (the counter the column goes to, its destination or -1, the vertices reached)."""
        W, keys = self.W, self.keys
        found, diagonals = self.exits(j, a, b)
        if diagonals:
            if len(diagonals) != 1:
                return "n_trace_failed", -1, 0
            other = [k for k in W.keys(*diagonals[0]) if k != keys[j]]
            o = self.owner(*diagonals[0], other[0])
            if o is None or o == j:
                return "n_trace_failed", -1, 0
            return ("n_traced", o, 0) if self.exits(o, a, b)[1] == diagonals else ("n_trace_failed", -1, 0)
        if len(found) != 1:
            return "n_trace_failed", -1, 0
        y, x, d = found[0]
        arrived, steps = OPPOSITE[d], 0
        while True:
            steps += 1
            if steps > max_trace:
                return "n_trace_overflow", -1, steps - 1
            if not W.in_range(y, x):
                return "n_trace_failed", -1, steps
            hold = [k for k in W.keys(y, x) if a in k and b in k]
            if hold:
                o = self.owner(y, x, hold[0])
                if o is None or o == j:
                    return "n_trace_failed", -1, steps
                theirs, diagonals = self.exits(o, a, b)
                return ("n_traced", o, steps) if not diagonals and len(theirs) == 1 else ("n_trace_failed", -1, steps)
            ab = [d for d, crack in enumerate(W.cracks(y, x)) if set(crack) == {a + 1, b + 1}]
            if len(ab) != 2 or arrived not in ab:
                return "n_trace_failed", -1, steps
            d = ab[0] if ab[1] == arrived else ab[1]
            y, x = W.norm(y + STEP[d][0], x + STEP[d][1])
            arrived = OPPOSITE[d]


def trace_links(W, triples, rep, jj, max_trace):
    """The open columns of one image's joint->joint list `jj` [2, 3 n] (local indices) traced in place.
    -> the three counters as a dict."""
    T = Tracer(W, triples, rep)
    counters = dict.fromkeys(COUNTERS, 0)
    before = jj[1].copy()
    for j in range(len(triples)):
        for k, (ia, ib) in enumerate(PAIRS):
            if before[3 * j + k] != -1:
                continue
            what, o, _ = T.partner(j, T.keys[j][ia], T.keys[j][ib], max_trace)
            counters[what] += 1
            jj[1, 3 * j + k] = o
    return counters


def vectorize(image, n_grain, grid="cells", merge_radius=2, joint_capacity=None, boundary="periodic", max_trace=None):
    """tests/vectorcheck.py's (periodic) or tests/vectorcheck_noflux.py's dict with the open pairs traced: jj and
    status["n_open_pairs"] afterwards, and in addition rep int32 [n], counters (dict), n_open_before."""
    one = vc.vectorize if boundary == "periodic" else vn.vectorize
    v = one(image, n_grain, grid, merge_radius=merge_radius, joint_capacity=joint_capacity)
    W = Windows(image, n_grain, merge_radius, boundary)
    n = len(v["triples"])
    reps = W.representatives()
    assert len(reps) == v["status"]["n_joint"] and [k for _, k in reps[:n]] == [tuple(t) for t in v["triples"].tolist()]
    v["rep"] = np.array([r for r, _ in reps[:n]], np.int32)
    v["n_open_before"] = v["status"]["n_open_pairs"]
    ny, nx = np.asarray(image).shape
    v["counters"] = trace_links(W, v["triples"], v["rep"], v["jj"], default_max_trace(ny, nx) if max_trace is None else int(max_trace))
    assert sum(v["counters"].values()) == v["n_open_before"]
    v["status"] = dict(v["status"], n_open_pairs=v["n_open_before"] - v["counters"]["n_traced"])
    return v


def is_valid(status, boundary):
    return (vc.is_valid if boundary == "periodic" else vn.is_valid)(status)


def vectorize_union(images, n_grains, grid="cells", merge_radius=2, joint_capacity=None, boundary="periodic", max_trace=None):
    """tests/vectorcheck_union.py's dict with every image's open pairs traced: image b keeps its first joint_capacity -
    joint_off[b] junctions and is traced with those (an owner that was cut off owns nothing).  In addition rep int32 [n] and
    counters, a list of dicts."""
    u = vu.vectorize(images, n_grains, grid, merge_radius, joint_capacity, boundary)
    n = len(u["triples"])
    ny, nx = np.asarray(images[0]).shape
    limit = default_max_trace(ny, nx) if max_trace is None else int(max_trace)
    u["rep"], u["counters"] = np.zeros(n, np.int32), []
    for b, image in enumerate(images):
        j0, j1, g0 = min(u["joint_off"][b], n), min(u["joint_off"][b + 1], n), u["grain_off"][b]
        W = Windows(image, n_grains[b], merge_radius, boundary)
        u["rep"][j0:j1] = [r for r, _ in W.representatives()[:j1 - j0]]
        own = u["jj"][:, 3 * j0:3 * j1].copy()
        own[1] = np.where(own[1] >= 0, own[1] - j0, own[1])
        c = trace_links(W, u["triples"][j0:j1] - np.int32(g0), u["rep"][j0:j1], own, limit)
        u["jj"][1, 3 * j0:3 * j1] = np.where(own[1] >= 0, own[1] + j0, own[1])
        u["counters"].append(c)
        u["status"][b] = dict(u["status"][b], n_open_pairs=u["status"][b]["n_open_pairs"] - c["n_traced"])
    return u
