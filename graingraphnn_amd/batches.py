"""Training on device-resident mini-batches.

The reference's training loop (train.py:365-366) shuffles its graphs and collates `batch_size` of them per step: every
batch has other node counts and other edge lists.  Here the samples are packed once into arenas on the device
(`DeviceDataset`), an epoch's order is a small table of sample ids, and one launch (`ggnn_collate_batch`) writes the batch a
device-side cursor points at into buffers of CAPACITY shape (`DeviceBatches`): addresses and shapes never change, so a
hipGraph captured on them (`training.GraphedTrainStep(model, optimizer, loss_fn, batches)`) replays over every batch of every
epoch.

The pad rule.  Node rows behind the batch's real ones are zeros with mask 0; the LAST row of every node type at capacity is
never a real node, and the edges behind the batch's real ones run from that row to that row.  The forward and the reverse
CSR are masked builds that skip it (`ggnn_csr_mask`), so pad edges are in no table, pad nodes are rows without edges, and the
tables' kept-edge word is the `E_dev` of the per-edge kernels.  Pad edges carry label -1 and edge_attr 0."""
from typing import Dict

import numpy as np
import torch

from . import _lib
from .backend import default_backend
from .engine import GraphCSR, register_inplace_graph
from .packing import EDGE_TYPES, NODE_TYPES

ET_JJ = ("joint", "connect", "joint")
KINDS = NODE_TYPES + EDGE_TYPES           # the row kinds an offset table exists for: node types, then edge types
NODE_SLACK = 1                            # the reserved last row of a node type (the pad edges' end points)


def _np(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _sample_parts(s):
    """A sample -> (x, edge_index, edge_attr, y, mask) dicts: a mapping with those keys (x_dict / edge_index_dict /
    edge_attr_dict / y_dict are accepted too), an object with such attributes, or the 5-tuple itself."""
    if isinstance(s, (tuple, list)) and len(s) == 5:
        return tuple(s)
    get = (lambda k: s.get(k)) if hasattr(s, "get") else (lambda k: getattr(s, k, None))
    parts = []
    for names in (("x", "x_dict"), ("edge_index", "edge_index_dict"), ("edge_attr", "edge_attr_dict"), ("y", "y_dict"),
                  ("mask",)):
        v = next((get(n) for n in names if get(n) is not None), None)
        if v is None:
            raise ValueError(f"a sample needs '{names[0]}'")
        parts.append(v)
    return tuple(parts)


def batch_capacity(sizes, batch_size: int, slack: int = 0) -> int:
    """Rows a batch buffer needs so that EVERY batch of `batch_size` different samples fits: the `batch_size` largest
    samples together, plus `slack` fixed rows; at least one row."""
    top = np.sort(np.asarray(sizes, dtype=np.int64))[::-1][:batch_size]
    return max(int(top.sum()) + slack, 1)


def order_table(perm, n_samples: int, batch_size: int) -> np.ndarray:
    """An epoch's order as int32 [n_batches, batch_size] sample ids, -1 = an empty slot: consecutive runs of `perm`, the
    last batch partial (the reference's DataLoader does not drop it).  `perm` must be a permutation of the samples: the
    capacities hold the `batch_size` largest DIFFERENT samples."""
    perm = np.asarray(_np(perm), dtype=np.int64).reshape(-1)
    if perm.size != n_samples or not np.array_equal(np.sort(perm), np.arange(n_samples)):
        raise ValueError(f"the order must be a permutation of the {n_samples} samples")
    n_batches = -(-n_samples // batch_size)
    table = np.full(n_batches * batch_size, -1, dtype=np.int32)
    table[:n_samples] = perm
    return table.reshape(n_batches, batch_size)


class DeviceDataset:
    """The samples of a training set packed once, on the device.  A sample is what the reference's
    `DynamicHeteroGraphTemporalSignal.__getitem__` yields (data_loader.py:113-162), as numpy arrays or tensors:
    x[nt] float32 [N, F]; edge_index[et] int64 [2, E] (local indices); edge_attr[et] float32 [E] or [E, 1]; y: grain [N_g, 2],
    joint [N_j, 2], edge_event [E_jj] int64 (-1 = unlabelled; absent: all -1), grain_event [N_g] (optional); mask: grain,
    joint ([N] or [N, 1], dtype kept: 4- or 8-byte elements).

    One arena per array (the rows of all samples one after another), per-sample offsets int64 [S + 1] per node type and per
    edge type (`offsets`, host; `offsets_dev`, device).  `capacity[kind]`: the `batch_size` largest samples together, plus the
    reserved row of a node type -- computed once, so every batch fits.  `set_order(perm)` uploads an epoch's order and resets
    the device cursor; the host keeps the table, so `sizes(b)` / `slices(b)` need no read-back."""

    def __init__(self, samples, batch_size: int, device="cuda"):
        samples = [_sample_parts(s) for s in samples]
        if not samples:
            raise ValueError("DeviceDataset: no samples")
        if not 1 <= batch_size <= _lib.GGNN_COLLATE_MAX_BATCH:
            raise ValueError(f"DeviceDataset: batch_size must be 1..{_lib.GGNN_COLLATE_MAX_BATCH}")
        self.n_samples, self.batch_size, self.device = len(samples), int(batch_size), torch.device(device)
        self.n_batches = -(-self.n_samples // self.batch_size)
        host: Dict[tuple, list] = {}
        sizes = {k: np.zeros(self.n_samples, np.int64) for k in KINDS}
        self.has_grain_event = all("grain_event" in s[3] for s in samples)
        for i, (x, ei, ea, y, mask) in enumerate(samples):
            for nt in NODE_TYPES:
                xa = np.ascontiguousarray(_np(x[nt]), dtype=np.float32)
                n = sizes[nt][i] = xa.shape[0]
                ya = np.ascontiguousarray(_np(y[nt]), dtype=np.float32)
                ma = np.ascontiguousarray(_np(mask[nt]))
                if ma.dtype == np.bool_ or ma.dtype.itemsize not in (4, 8):
                    ma = ma.astype(np.float32)
                if xa.ndim != 2 or ya.shape != (n, 2) or ma.size != n:
                    raise ValueError(f"sample {i}: x['{nt}'] [N, F], y['{nt}'] [N, 2] and mask['{nt}'] [N] or [N, 1] must agree")
                host.setdefault(("x", nt), []).append(xa)
                host.setdefault(("y", nt), []).append(ya)
                host.setdefault(("mask", nt), []).append(ma)
            if self.has_grain_event:
                ge = np.ascontiguousarray(_np(y["grain_event"]))
                if ge.shape != (sizes["grain"][i],) or ge.dtype.itemsize not in (4, 8):
                    raise ValueError(f"sample {i}: y['grain_event'] must hold one 4- or 8-byte element per grain")
                host.setdefault(("y", "grain_event"), []).append(ge)
            for et in EDGE_TYPES:
                e = np.ascontiguousarray(_np(ei[et]), dtype=np.int64)
                a = np.ascontiguousarray(_np(ea[et]), dtype=np.float32)
                if e.ndim != 2 or e.shape[0] != 2 or a.size != e.shape[1] or a.shape[0] != e.shape[1]:
                    raise ValueError(f"sample {i}: edge_index[{et}] [2, E] and edge_attr[{et}] [E] or [E, 1] must agree")
                if e.size and (e.min() < 0 or e[0].max() >= sizes[et[0]][i] or e[1].max() >= sizes[et[-1]][i]):
                    raise IndexError(f"sample {i}: edge_index[{et}] has entries outside the sample's nodes")
                sizes[et][i] = e.shape[1]
                host.setdefault(("edge_index", et), []).append(e)
                host.setdefault(("edge_attr", et), []).append(a)
            lab = y.get("edge_event") if hasattr(y, "get") else None
            lab = np.full(sizes[ET_JJ][i], -1, np.int64) if lab is None else np.ascontiguousarray(_np(lab), dtype=np.int64)
            if lab.shape != (sizes[ET_JJ][i],):
                raise ValueError(f"sample {i}: y['edge_event'] must hold one label per junction-junction edge")
            host.setdefault(("y", "edge_event"), []).append(lab)
        for key, parts in host.items():
            if key[0] != "edge_index" and len({(p.dtype, p.shape[1:]) for p in parts}) != 1:
                raise ValueError(f"the samples' {key} differ in dtype or trailing shape")
        self.sizes_by_sample = sizes
        self.offsets = {k: np.concatenate([[0], np.cumsum(sizes[k])]).astype(np.int64) for k in KINDS}
        self.capacity = {k: batch_capacity(sizes[k], self.batch_size, NODE_SLACK if k in NODE_TYPES else 0) for k in KINDS}
        dev = self.device
        # the arenas: rows of all samples one after another; an edge list's two rows are the arena's two rows
        self.arena = {key: torch.from_numpy(np.concatenate(parts, 1 if key[0] == "edge_index" else 0)).contiguous().to(dev)
                      for key, parts in host.items()}
        self.offsets_dev = torch.from_numpy(np.stack([self.offsets[k] for k in KINDS])).to(dev)   # [5, S + 1]
        self.order_dev = torch.empty(self.n_batches, self.batch_size, dtype=torch.int32, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self.sync_word = torch.zeros(1, dtype=torch.int32, device=dev)
        self.order = None
        self.position = 0   # the host's copy of the cursor: batches collated since set_order
        self.set_order(np.arange(self.n_samples))

    def set_order(self, perm):
        """Upload an epoch's order (a host permutation of the sample ids, e.g. torch.randperm with the caller's generator)
        into the table the collation reads -- in place: a captured step stays valid -- and reset the cursor to batch 0."""
        self.order = order_table(perm, self.n_samples, self.batch_size)
        self.order_dev.copy_(torch.from_numpy(self.order))
        self.cursor.zero_()
        self.position = 0

    def batch_ids(self, b: int):
        """The sample ids of batch b (the empty slots left out)."""
        row = self.order[int(b) % self.n_batches]
        return [int(i) for i in row if i >= 0]

    def sizes(self, b: int):
        """{node type / edge type: real rows / edges of batch b} from the host's table."""
        ids = self.batch_ids(b)
        return {k: int(self.sizes_by_sample[k][ids].sum()) for k in KINDS}

    def slices(self, b: int):
        """Per sample of batch b its row range per node type and its edge range per edge type: the `slices` of
        synthetic.disjoint_union, with the edge types' ranges beside the node types'."""
        at = {k: 0 for k in KINDS}
        out = []
        for i in self.batch_ids(b):
            out.append({k: (at[k], at[k] + int(self.sizes_by_sample[k][i])) for k in KINDS})
            for k in KINDS:
                at[k] += int(self.sizes_by_sample[k][i])
        return out

    def _advanced(self):
        self.position += 1


class _InPlaceTopology:
    """training.TrainTopology's interface on tables that `DeviceBatches.next()` refills in place."""

    def __init__(self, graph, rcsr, r_slot):
        self.graph, self.rcsr, self.r_slot = graph, rcsr, r_slot

    def jj_index(self):
        """As TrainTopology.jj_index, made anew per call (the tables change under the same addresses), over all slots of the
        capacity: behind the kept ones `slot_edge` and `r_slot` hold 0 -- valid indices --, and the row pointers end at the
        kept count, so the segment sums of the classifier heads' backward never reach them."""
        csr, rcsr = self.graph.csr[ET_JJ], self.rcsr[ET_JJ]
        return {"slot_edge": csr.perm.long(), "rowptr": csr.rowptr.long(),
                "r_slot": self.r_slot[ET_JJ].long(), "r_rowptr": rcsr.rowptr.long()}


class DeviceBatches:
    """The batch buffers of a `DeviceDataset` and everything the models need on them: `x_dict`, `edge_index_dict`,
    `edge_attr`, `y_dict`, `mask` in the layout of synthetic.disjoint_union in their leading part and padded to the
    dataset's capacities (module docstring); `counts[kind]` / `rows[nt]` int64 [1] device words with the real rows and edges,
    `batch_offsets` int64 [5, batch_size + 1] the first row / edge of every sample.  `next()` = the collation of the batch at
    the dataset's cursor plus the rebuild of the forward and reverse tables, all in place and without a read-back; the
    cursor advances on the device.  The reference-shaped calls work on the dicts as they are:

        batches.next()
        loss = regressor_loss(batches.y_dict, model(batches.x_dict, batches.edge_index_dict, batches.edge_attr),
                              batches.mask, rows=batches.rows)

    (`graph_for` / `train_topology` answer the list tensors with the in-place tables.)  In .eval() mode the same call is
    the fused inference path; rows with mask 0 and labels -1 count nowhere in metrics.feature_metric.record."""

    def __init__(self, dataset: DeviceDataset):
        self.dataset = ds = dataset
        self.be = be = default_backend()
        dev, cap, B = ds.device, ds.capacity, ds.batch_size
        self.capacity = dict(cap)
        self._counts = torch.zeros(len(KINDS), dtype=torch.int64, device=dev)
        self.batch_offsets = torch.zeros(len(KINDS), B + 1, dtype=torch.int64, device=dev)
        self.counts = {k: self._counts[i:i + 1] for i, k in enumerate(KINDS)}
        self.rows = {nt: self.counts[nt] for nt in NODE_TYPES}
        buf = {}
        for key, arena in ds.arena.items():
            k = key[1] if key[1] in KINDS else ("grain" if key[1] == "grain_event" else ET_JJ)
            if key[0] == "edge_index":
                pad = torch.tensor([[cap[k[0]] - 1], [cap[k[-1]] - 1]], dtype=torch.int64, device=dev)
                buf[key] = pad.expand(2, cap[k]).contiguous()
            else:
                buf[key] = torch.full((cap[k],) + tuple(arena.shape[1:]), -1 if key == ("y", "edge_event") else 0,
                                      dtype=arena.dtype, device=dev)
        self._buf = buf
        self._ei_flipped = {et: buf[("edge_index", et)].flip(0).contiguous() for et in EDGE_TYPES}
        self.x_dict = {nt: buf[("x", nt)] for nt in NODE_TYPES}
        self.edge_index_dict = {et: buf[("edge_index", et)] for et in EDGE_TYPES}
        self.edge_attr = {et: buf[("edge_attr", et)] for et in EDGE_TYPES}
        self.y_dict = {nt: buf[("y", nt)] for nt in NODE_TYPES}
        self.y_dict["edge_event"] = buf[("y", "edge_event")]
        if ds.has_grain_event:
            self.y_dict["grain_event"] = buf[("y", "grain_event")]
        self.mask = {nt: buf[("mask", nt)] for nt in NODE_TYPES}
        self._args = self._collate_args()
        # the tables, forward and reverse: masked builds that skip the reserved rows, refilled in place by next()
        shapes = [(cap[et], cap[et[0]], cap[et[-1]]) for et in EDGE_TYPES]
        self._fwd = be.csr_in_place(shapes, dev, masks=[(cap[et[0]] - 1, cap[et[-1]] - 1) for et in EDGE_TYPES])
        self._rev = be.csr_in_place([(e, d, s) for e, s, d in shapes], dev,
                                    masks=[(cap[et[-1]] - 1, cap[et[0]] - 1) for et in EDGE_TYPES])
        self._fwd_lists = [self.edge_index_dict[et] for et in EDGE_TYPES]
        self._rev_lists = [self._ei_flipped[et] for et in EDGE_TYPES]
        n_nodes = {nt: cap[nt] for nt in NODE_TYPES}
        self.graph = GraphCSR(be, self.edge_index_dict, n_nodes, into=self._fwd,
                              counts=dict(zip(EDGE_TYPES, self._fwd.kept)))
        rcsr = dict(zip(EDGE_TYPES, self._rev.rebuild(self._rev_lists)))
        self._r_slot = {et: torch.zeros(cap[et], dtype=torch.int32, device=dev) for et in EDGE_TYPES}
        self._scratch = {et: torch.zeros(cap[et], dtype=torch.int32, device=dev) for et in EDGE_TYPES}
        self.topology = self.graph.train_topology = _InPlaceTopology(self.graph, rcsr, self._r_slot)
        self._slot_items = [(self.graph.csr[et], rcsr[et], self._r_slot[et], self._scratch[et]) for et in EDGE_TYPES]
        register_inplace_graph(self.graph)

    def _collate_args(self):
        ds, cap = self.dataset, self.capacity
        a = _lib.CollateArgs()
        S1 = ds.n_samples + 1
        for i in range(len(KINDS)):
            a.sample_off[i] = ds.offsets_dev.data_ptr() + 8 * S1 * i
            a.batch_off[i] = self.batch_offsets.data_ptr() + 8 * (ds.batch_size + 1) * i
            a.count[i] = self._counts.data_ptr() + 8 * i
        a.order, a.sync_word = ds.order_dev.data_ptr(), ds.sync_word.data_ptr()
        a.cursor_in = a.cursor_out = ds.cursor.data_ptr()
        n_rows = n_lists = 0
        owner = set()   # the first array of a node kind writes the kind's count and offsets
        for key, arena in ds.arena.items():
            if key[0] == "edge_index":
                continue
            k = key[1] if key[1] in KINDS else ("grain" if key[1] == "grain_event" else ET_JJ)
            r, dst = a.rows[n_rows], self._buf[key]
            row_bytes = arena.element_size() * int(np.prod(arena.shape[1:], dtype=np.int64))
            if row_bytes % 4 or n_rows >= _lib.GGNN_COLLATE_MAX_ROWS:
                raise _lib.GGNNError("DeviceBatches: row arrays of 4-byte words, at most %d of them" % _lib.GGNN_COLLATE_MAX_ROWS)
            r.src, r.dst, r.cap, r.words, r.kind = arena.data_ptr(), dst.data_ptr(), cap[k], row_bytes // 4, KINDS.index(k)
            r.pad_word = 0xFFFFFFFF if key == ("y", "edge_event") else 0
            r.meta = int(k in NODE_TYPES and k not in owner)
            owner.add(k)
            n_rows += 1
        for et in EDGE_TYPES:
            l, arena = a.lists[n_lists], ds.arena[("edge_index", et)]
            l.src, l.dst, l.dst_flipped = arena.data_ptr(), self._buf[("edge_index", et)].data_ptr(), self._ei_flipped[et].data_ptr()
            l.ld_src, l.cap = arena.size(1), cap[et]
            l.pad_src, l.pad_dst = cap[et[0]] - 1, cap[et[-1]] - 1
            l.kind, l.kind_src, l.kind_dst = KINDS.index(et), KINDS.index(et[0]), KINDS.index(et[-1])
            n_lists += 1
        a.n_samples, a.n_batches, a.batch_size = ds.n_samples, ds.n_batches, ds.batch_size
        a.n_kinds, a.n_rows, a.n_lists = len(KINDS), n_rows, n_lists
        return a

    def next(self):
        """Collate the batch at the cursor into the buffers and rebuild the tables on it: one collation launch, two masked
        CSR builds (forward, reverse) and the reverse-slot kernels, all on the current stream; capturable.  Returns self."""
        be = self.be
        be.collate_batch(self._args)
        self._fwd.rebuild(self._fwd_lists)
        self._rev.rebuild(self._rev_lists)
        be.reverse_slots(self._slot_items)
        if not torch.cuda.is_current_stream_capturing():   # (a capture records the launches; a replay counts in _advanced)
            self.dataset._advanced()
        return self

    def _advanced(self):
        self.dataset._advanced()

    @property
    def current(self):
        """Index of the batch that stands in the buffers (by the host's count of collations since set_order)."""
        return (self.dataset.position - 1) % self.dataset.n_batches

    def sizes(self, b=None):
        return self.dataset.sizes(self.current if b is None else b)

    def slices(self, b=None):
        return self.dataset.slices(self.current if b is None else b)
