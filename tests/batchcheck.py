"""numpy restatement of training on device-resident mini-batches: the order table, the capacity rule, the padded
collation of `ggnn_collate_batch`, and the masked forward / reverse tables with their reverse slots -- written from the
description in include/ggnn.h, sharing no code with graingraphnn_amd/batches.py -- plus the seven-sample dataset the tests of
tests/test_training_device_batches.py run on."""
import itertools
import os

import numpy as np

from helpers import EDGE_TYPES, GOLDEN
from graingraphnn_amd import synthetic

NODE_TYPES = ("grain", "joint")
KINDS = NODE_TYPES + tuple(EDGE_TYPES)
ET_JJ = EDGE_TYPES[2]
BATCH = 3


def _fixture(name):
    return synthetic.load_fixture(os.path.join(GOLDEN, name + ".npz"))


def make_samples(extra_large=False):
    """Seven samples of four sizes: graph_40, two generated 40 um structures, the no-flux structure taken as a plain graph
    (its grain 0 has a large in-degree) and three perturbed copies of graph_40; targets and masks as
    test_training._targets draws them (grain masks with zeros, junction-edge labels -1 / 0 / 1), grain events 0 / 1.
    extra_large: an eighth, larger sample (generated_80_seed7) that only inflates the capacities."""
    from test_training import _targets
    x0, ei0, ea0 = _fixture("graph_40")
    graphs = [(x0, ei0, ea0), _fixture("generated_40_seed1"), _fixture("generated_40_seed2"), _fixture("noflux_40_seed1")]
    graphs += [(synthetic.perturbed_copy(x0, 1e-3, 2000 + t), ei0, ea0) for t in range(3)]
    if extra_large:
        graphs.append(_fixture("generated_80_seed7"))
    samples = []
    for i, (x, ei, ea) in enumerate(graphs):
        y, mask = _targets(x, ei)
        y["grain_event"] = np.random.RandomState(300 + i).randint(0, 2, size=x["grain"].shape[0]).astype(np.int64)
        samples.append({"x": x, "edge_index": ei, "edge_attr": ea, "y": y, "mask": mask})
    return samples


def size_of(sample, kind):
    return sample["x"][kind].shape[0] if kind in NODE_TYPES else sample["edge_index"][kind].shape[1]


def capacity(samples, batch_size=BATCH):
    """Per kind: the batch_size largest samples together; a node type has one more row, the reserved last one."""
    cap = {}
    for k in KINDS:
        sizes = sorted((size_of(s, k) for s in samples), reverse=True)
        cap[k] = max(sum(sizes[:batch_size]) + (1 if k in NODE_TYPES else 0), 1)
    return cap


def order_table(perm, batch_size=BATCH):
    perm = list(perm)
    n_batches = -(-len(perm) // batch_size)
    rows = []
    for b in range(n_batches):
        ids = perm[b * batch_size:(b + 1) * batch_size]
        rows.append(ids + [-1] * (batch_size - len(ids)))
    return np.array(rows, dtype=np.int32)


def union(samples, ids):
    """The host collation of the reference's loop: synthetic.disjoint_union plus the concatenated targets and masks."""
    picked = [samples[i] for i in ids]
    x, ei, ea, slices = synthetic.disjoint_union([(s["x"], s["edge_index"], s["edge_attr"]) for s in picked])
    y = {k: np.concatenate([s["y"][k] for s in picked], 0) for k in ("grain", "joint", "edge_event", "grain_event")}
    mask = {nt: np.concatenate([s["mask"][nt] for s in picked], 0) for nt in NODE_TYPES}
    return x, ei, ea, y, mask, slices


def collate(samples, ids, cap):
    """The padded batch: the union in the leading part; behind it node rows of zeros with mask 0, edges from the reserved
    row to the reserved row with edge_attr 0 and label -1.  -> dict of arrays keyed like DeviceBatches' buffers, `counts`
    {kind: n}, `offsets` {kind: [len(ids) + 1]}."""
    x, ei, ea, y, mask, _ = union(samples, ids)
    out = {}

    def padded(a, n, fill=0):
        full = np.full((n,) + a.shape[1:], fill, dtype=a.dtype)
        full[:a.shape[0]] = a
        return full
    for nt in NODE_TYPES:
        out[("x", nt)] = padded(x[nt], cap[nt])
        out[("y", nt)] = padded(y[nt], cap[nt])
        out[("mask", nt)] = padded(mask[nt], cap[nt])
    out[("y", "grain_event")] = padded(y["grain_event"], cap["grain"])
    out[("y", "edge_event")] = padded(y["edge_event"], cap[ET_JJ], -1)
    for et in EDGE_TYPES:
        full = np.empty((2, cap[et]), np.int64)
        full[0], full[1] = cap[et[0]] - 1, cap[et[-1]] - 1
        full[:, :ei[et].shape[1]] = ei[et]
        out[("edge_index", et)] = full
        out[("edge_attr", et)] = padded(ea[et], cap[et])
    counts = {k: sum(size_of(samples[i], k) for i in ids) for k in KINDS}
    offsets = {k: np.concatenate([[0], np.cumsum([size_of(samples[i], k) for i in ids])]).astype(np.int64) for k in KINDS}
    return out, counts, offsets


def csr(edge_index, n_dst, skip=None):
    """Destination-grouped table of a list [2, E] without the edges from skip[0] / into skip[1]: rowptr [n_dst + 1], and over
    the kept slots perm (original edge, rising inside a row), col (source) and row (destination)."""
    src, dst = edge_index
    keep = np.ones(src.shape[0], bool) if skip is None else (src != skip[0]) & (dst != skip[1])
    e = np.flatnonzero(keep)
    perm = e[np.argsort(dst[e], kind="stable")]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst[e], minlength=n_dst))])
    return {"rowptr": rowptr.astype(np.int64), "perm": perm.astype(np.int64), "col": src[perm], "row": dst[perm],
            "kept": int(e.size)}


def tables(edge_index, n_src, n_dst, skip=None):
    """Forward table, reverse (source-grouped) table of the flipped list, and r_slot: the forward slot of every reverse slot."""
    fwd = csr(edge_index, n_dst, skip)
    rev = csr(edge_index[::-1], n_src, None if skip is None else skip[::-1])
    inv = np.full(edge_index.shape[1], -1, np.int64)
    inv[fwd["perm"]] = np.arange(fwd["kept"])
    return fwd, rev, inv[rev["perm"]]


def three_subsets(n, k=BATCH):
    return itertools.combinations(range(n), k)
