"""Shared checking code of the fused forward cells (ggnn_decoder_cell_batch / ggnn_encoder_cell_batch): the fp64
restatement of one HeteroPGCLSTM cell from the ORIGINAL fp32 weights, a cell problem built at the sweep's edges, and
per-element error magnitudes of (h, c).

Bounds are per element, against the fp64 magnitude of that element's own sum pushed through the LSTM update (never
against a tensor's largest entry): an output of 1e-3 is held to its own size.  The tolerance is gradcheck's SWEEP_TOL;
it is fixed by the reference -- the torch CPU float32 evaluation of the same formulas stays at <= 0.5 of the bound on
every element (tests/test_forward_cells.py, on a CPU alone) -- never by the kernel under test.

Measured worst |got - ref64| / bound per case (<= 1 passes; HIP on an MI355X, the fused cell and -- decoder -- the split
plan's kernels, beside the torch CPU float32 restatement, which must stay <= 0.5):
    dec-n_in2-n_dst373                   fused 0.079   split plan 0.079   fp32 restatement 0.015
    dec-n_in2-second_empty-n_dst373      fused 0.095   split plan 0.095   fp32 restatement 0.031
    dec-n_in1-n_dst373                   fused 0.079   split plan 0.079   fp32 restatement 0.031
    dec-n_in2-n_dst5                     fused 0.053   split plan 0.053   fp32 restatement 0.004
    enc-n_in2-n_dst373                   fused 0.065   split plan   -     fp32 restatement 0.008
    enc-n_in2-second_empty-n_dst373      fused 0.083   split plan   -     fp32 restatement 0.010
    enc-n_in1-n_dst373                   fused 0.085   split plan   -     fp32 restatement 0.009
    enc-n_in2-n_dst5                     fused 0.034   split plan   -     fp32 restatement 0.003
The worst HIP elements all lie in the small output channels (90 .. 95), where the read-out floor of the hardware exp / rcp
units is most of the bound: the same element and figure for the fused cell and the split plan, whose gates share that
read-out.  Forward columns of the split sweep (test_hip_sweep_backward_against_fp64; HIP / fp32 restatement): aggregate
0.080 / 0.096 (decoder) and 0.064 / 0.116 (encoder), sum alpha 0.002 / 0.026 and 0.003 / 0.034, sum alpha a 0.035 / 0.030
and 0.023 / 0.032.
"""
import numpy as np
import torch

import gradcheck as gc

C = 96


# --------------------------------------------------------------------------------------------------------------------
# The fp64 restatement and the wide-range problem (shared with tests/test_hip_parity.py)
# --------------------------------------------------------------------------------------------------------------------
def _wide(rs, shape, lo, hi, signed=True):
    """Magnitudes 10^U(lo, hi), element by element (a dynamic range no single scale has), random signs."""
    v = 10.0 ** rs.uniform(lo, hi, shape)
    if signed:
        v = v * rs.choice([-1.0, 1.0], shape)
    return torch.from_numpy(v.astype(np.float32))


def _cell_reference(kind, P, dtype):
    """One HeteroPGCLSTM cell of the contract (include/ggnn.h), evaluated on the CPU in `dtype` from the ORIGINAL fp32
    operands and weights of `P` -- nothing decoded from a weight stream: what the reference formulation computes.
    kind = "dec" (h, c given; four gates) or "enc" (zero state; three gates)."""
    t = lambda v: v.cpu().to(dtype)
    x, n = t(P["x_dst"]), P["x_dst"].size(0)
    G = 4 if kind == "dec" else 3
    if kind == "dec":
        xin = torch.cat([t(P["h_dst"]), x, torch.ones(n, 1, dtype=dtype)], 1)                  # [h | x | 1]
    else:
        xin = torch.cat([x, torch.ones(n, 1, dtype=dtype)], 1)                                # [x | 1]
    pre = []
    for g in range(G):
        z = xin @ t(P["skip"][g]).t()
        for d, sw in enumerate(P["sweeps"]):
            rowptr = sw["rowptr"].cpu().long()
            E = int(rowptr[-1])
            dst = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
            src = sw["col"].cpu().long()[:E]
            einfo = t(sw["einfo"])
            x4, reloc, a = einfo[:E, :16], einfo[:E, 16:19], einfo[:E, 19]
            u = xin @ t(sw["score"][g]).t()                                                    # dec: [n, 96 + 16]; enc: [n, 16]
            if kind == "dec":
                sc = (u[dst, :96] * t(sw["h_src"])[src]).sum(-1) + (u[dst, 96:] * x4).sum(-1)
                val = torch.relu(t(sw["v_src"])[src][:, sw["v_off"] + g * 96: sw["v_off"] + (g + 1) * 96] + reloc @ t(sw["ep"])[g])
            else:
                sc = (u[dst] * x4).sum(-1)
                val = torch.relu(x4 @ t(sw["value"][g]).t())
            smax = torch.full((n,), float("-inf"), dtype=dtype).scatter_reduce(0, dst, sc, "amax")
            p = (sc - smax[dst]).exp()
            den = torch.zeros(n, dtype=dtype).index_add(0, dst, p)
            alpha = p / (den[dst] + 1e-16)
            A = torch.zeros(n, 96, dtype=dtype).index_add(0, dst, alpha[:, None] * val)
            sa = torch.zeros(n, dtype=dtype).index_add(0, dst, alpha)
            sae = torch.zeros(n, dtype=dtype).index_add(0, dst, alpha * a)
            z = z + A @ t(sw["l2"][g]).t() + sa[:, None] * t(sw["b_l2"][g])[None] + sae[:, None] * t(sw["w_edge"][g])[None]
        pre.append(z)
    if kind == "dec":
        c = torch.sigmoid(pre[1]) * t(P["c_in"]) + torch.sigmoid(pre[0]) * torch.tanh(pre[2])
        return torch.sigmoid(pre[3]) * torch.tanh(c), c
    c = torch.sigmoid(pre[0]) * torch.tanh(pre[1])
    return torch.sigmoid(pre[2]) * torch.tanh(c), c


def _wide_cell_problem(be, kind, rs, n_dst, ins, F_dst, with_edges=True, dev="cuda"):
    """A decoder / encoder cell problem whose operands span 1e-4 .. 1e2 element by element, with weights scaled so that
    the pre-activations stay O(1), on `dev` (where `be` builds its tables; _rebuild_wide_call follows P's device).
    Returns (the C-ABI call tuple, the dict of ORIGINAL fp32 operands and weights)."""
    G = 4 if kind == "dec" else 3
    d_ = lambda v: v.to(dev)
    xd = _wide(rs, (n_dst, F_dst), -4, 2, signed=False)
    P = {"x_dst": d_(xd), "sweeps": []}
    K = (96 if kind == "dec" else 0) + F_dst + 1
    if kind == "dec":
        P["h_dst"] = d_(torch.tanh(_wide(rs, (n_dst, 96), -4, 0.5)))
        P["c_in"] = d_(_wide(rs, (n_dst, 96), -4, 0.3))
    # every weight row is scaled by what it multiplies, so that sum |x||w| ~ 1 .. 10 per output
    feat_scale = 1.0 / (float(xd.abs().mean()) * F_dst + (30.0 if kind == "dec" else 0.0) + 1.0)
    wrow = lambda rows, cols, s: _wide(rs, (rows, cols), -2, 0) * s
    P["skip"] = [d_(wrow(96, K, feat_scale)) for _ in range(G)]
    for d, (n_src, F, E) in enumerate(ins):
        E = E if with_edges else 0
        src = rs.randint(0, max(n_src - 5, 1), size=E)
        dst = rs.randint(1 if n_dst > 1 else 0, n_dst, size=E)
        ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64)).to(dev)
        xs = _wide(rs, (n_src, F), -4, 2, signed=False)
        xs[:, :3] = torch.from_numpy(rs.uniform(0, 1, (n_src, 3)).astype(np.float32))   # coordinates stay in the unit box
        ea = torch.from_numpy(rs.uniform(0.01, 0.1, E).astype(np.float32)).to(dev)
        csr = be.build_csr(ei, n_src, n_dst)
        einfo = torch.zeros(E + 3, 20, device=dev)
        be.edge_prepare([(csr, ea, d_(xs), P["x_dst"], einfo)])
        rec_scale = 1.0 / (float(xs[:, 3:].abs().mean()) * max(F - 3, 1) + 2.0)
        sw = {"rowptr": csr.rowptr, "col": csr.col, "einfo": einfo, "csr": csr,
              "l2": [d_(wrow(96, 96, 0.05)) for _ in range(G)], "b_l2": [d_(wrow(96, 1, 0.3)[:, 0]) for _ in range(G)],
              "w_edge": [d_(wrow(96, 1, 0.3)[:, 0]) for _ in range(G)]}
        if kind == "dec":
            sw["h_src"] = d_(torch.tanh(_wide(rs, (n_src, 96), -4, 0.5)))
            sw["v_src"] = d_(_wide(rs, (n_src, 384 * (d + 1) + 96), -4, 1))
            sw["v_off"] = 384 * d
            sw["ep"] = d_(_wide(rs, (4, 3, 96), -2, 0))
            score = []
            for g in range(G):
                W1 = torch.zeros(112, K)
                W1[:96] = wrow(96, K, 0.02 * feat_scale)            # u_h rows (they meet h_src in (-1, 1))
                W1[96:110] = wrow(14, K, rec_scale * feat_scale)     # u4 rows (they meet the edge record)
                score.append(d_(W1))
            sw["score"] = score
        else:
            score, value = [], []
            for g in range(G):
                T = torch.zeros(16, K)
                T[:14] = wrow(14, K, rec_scale * feat_scale)
                if F <= 11:
                    T[11] = 0
                V = torch.zeros(96, 16)
                V[:, :F], V[:, 12] = wrow(96, F, rec_scale), wrow(96, 1, 0.3)[:, 0]
                score.append(d_(T))
                value.append(d_(V))
            sw["score"], sw["value"] = score, value
        P["sweeps"].append(sw)
    return _rebuild_wide_call(be, kind, P)


def _rebuild_wide_call(be, kind, P):
    """(call tuple, P): the operands and ORIGINAL weights of `P` in the kernels' weight-stream image; again after an
    in-place edit of the weights.  Everything stays on the device of P's tensors."""
    from graingraphnn_amd.packing import CELL_P3_CHANNEL, DC_GATE_ORDER, _plane_slices, _spread16
    G = 4 if kind == "dec" else 3
    dev = P["x_dst"].device
    n_dst, F_dst = P["x_dst"].shape
    n_in = len(P["sweeps"])
    K = (96 if kind == "dec" else 0) + F_dst + 1
    p3 = torch.tensor(CELL_P3_CHANNEL, device=dev)

    def in128(W):
        out = torch.zeros(W.size(0), 128, device=dev)
        out[:, :K] = W
        return out

    def slots16(W):
        out = torch.zeros(W.size(0), 16, device=dev)
        out[:, :F_dst], out[:, 12] = W[:, :F_dst], W[:, F_dst]
        return out

    slices = []
    for gi, g in enumerate(DC_GATE_ORDER if kind == "dec" else range(3)):
        for sw in (P["sweeps"][::-1] if kind == "dec" and gi & 1 else P["sweeps"]):   # decoder: backwards for the 2nd / 4th gate
            if kind == "dec":
                slices += [_plane_slices(in128(sw["score"][g])), _plane_slices(sw["l2"][g])]
            else:
                slices += [_plane_slices(_spread16(torch.cat([sw["value"][g], slots16(sw["score"][g])]))),
                           _plane_slices(sw["l2"][g][:, p3].contiguous())]
        slices.append(_plane_slices(in128(P["skip"][g]) if kind == "dec" else _spread16(slots16(P["skip"][g]))))
    wstream = torch.cat(slices).contiguous().view(-1)
    tail = torch.zeros(G, n_in, 6, 4, 16, device=dev)
    for d, sw in enumerate(P["sweeps"]):
        for g in range(G):
            tail[g, d, :, 0] = sw["b_l2"][g].view(6, 16)
            tail[g, d, :, 1 if kind == "dec" else 3] = sw["w_edge"][g].view(6, 16)
    tail = tail.view(G, n_in, 6, 64).contiguous()
    out = [torch.empty(n_dst, 96, device=dev), torch.empty(n_dst, 96, device=dev)]
    if kind == "dec":
        return ([(sw["csr"], sw["einfo"], sw["h_src"], sw["v_src"], sw["v_off"], sw["ep"]) for sw in P["sweeps"]],
                P["x_dst"], P["h_dst"], P["c_in"], wstream, tail, *out), P
    return ([(sw["csr"], sw["einfo"]) for sw in P["sweeps"]], P["x_dst"], wstream, tail, *out), P


# --------------------------------------------------------------------------------------------------------------------
# A cell problem at the sweep's edges
# --------------------------------------------------------------------------------------------------------------------
ROTATION = np.array([0, 1, 2, 3, 4, 6, 7])     # in-degrees in rotation: no, one and several units of GGNN_UNIT_EDGES = 3
WINDOW_TILES, WINDOW_LO = 21, 100               # aligned 16-row tiles with 100 .. 120 in-edges of the first edge type
N_DST, N_TINY = 373, 5                          # three workgroups of 128 rows, a last tile that slides back; < 16 rows
F_DST = 8
# destination feature columns: 0..2 coordinates, 3 "wide" indicator, 4 / 5 "+offset" / "-offset" indicators, 6..7 random
COL_WIDE, COL_UP, COL_DOWN = 3, 4, 5
FREE_COLS = (0, 1, 2, 6, 7)
KINDS = ("random", "wide, maximum on the first slot", "wide, maximum on the last slot", "all equal (u = 0)",
         "offset +300", "offset -300")
SMALL_CHANNELS = 6   # the last output channels: every weight row (and c_in) a hundred times smaller
WIDE_A, OFFSET, OFFSET_SPREAD = 800.0, 300.0, 20.0   # u4[13] = 800 on a in 0.01 .. 0.1: scores over +-36


def _units(deg):
    return (np.asarray(deg) + 2) // 3


def _degrees(n_dst, d):
    """In-degrees of edge type `d` (see cell_problem) and the rows it names: {"hub112", "hub900", "remainder": [...]}."""
    r = np.arange(n_dst)
    named = {"remainder": []}
    if n_dst < 16:
        deg = np.array([[7, 0, 4, 1, 6], [1, 3, 0, 7, 2]][d])[r % 5]
        return deg, named
    assert n_dst >= 16 * WINDOW_TILES + 32 and n_dst % 16 != 0
    deg = ROTATION[(r + 3 * d) % 7].copy()
    if d == 0:
        for t in range(WINDOW_TILES):
            b = 16 * t
            deg[b + 15] = 1                                     # exactly one edge at the tile's last CSR position
            if _units(deg[b + 11]) == 1:
                deg[b + 11] = 6                                 # the row in flight with it: another number of units
            deg[b + 7] = 0
            deg[b + 7] = WINDOW_LO + t - deg[b:b + 16].sum()    # the tile's total: 100 + t
            named["remainder"].append(b + 7)
        named["hub112"], named["hub900"] = 16 * WINDOW_TILES, n_dst - 1   # a tile's first row; the last row of the slid-back tile
    else:
        named["hub112"], named["hub900"] = 48, 16 * WINDOW_TILES + 14     # (inside one of the first type's window tiles)
    deg[named["hub112"]], deg[named["hub900"]] = 112, 900
    # the two rows of a pair in flight (tile rows 8 half + kq and + 4): different numbers of units, in the aligned tiles
    # and in the last one, which slides back to n_dst - 16
    for row0 in list(range(0, n_dst - 15, 16)) + [n_dst - 16]:
        for i in (0, 1, 2, 3, 8, 9, 10, 11):
            assert _units(deg[row0 + i]) != _units(deg[row0 + i + 4]), (d, row0, i)
    return deg, named


def _x4_64(xs, xd, src, dst, ea, F):
    """The edge records' 16 slots in fp64 from the coordinates and features (as ggnn_edge_prepare forms them)."""
    E = src.size
    x4 = np.zeros((E, 16))
    x4[:, :3] = gc.min_image(torch.from_numpy(xs[src, :3]).double(), torch.from_numpy(xd[dst, :3]).double()).numpy()
    x4[:, 3:F] = xs[src, 3:F]
    if F <= 11:
        x4[:, 11] = 1.0
    x4[:, 12], x4[:, 13] = 1.0, ea
    return x4


def cell_problem(kind, seed, n_in, n_dst=N_DST, empty_second=False, be=None, dev="cpu"):
    """A decoder ("dec") / encoder ("enc") cell problem at the sweep's edges, as a `P` dict in _rebuild_wide_call's
    format (plus, per sweep, its edge list "ei" in COO order, "ea", "xs" and "n_src", and P["meta"]).  `be` builds the
    CSR tables and the edge records on `dev` (default: the torch emulator on the CPU).

    Rows: n_dst = 373 (three workgroups of 128, n_dst % 16 = 5: the last tile slides back) or 5 (fewer than 16 rows).
    In-degrees 0, 1, 2, 3, 4, 6, 7 in rotation, the two rows of a pair in flight always with different numbers of
    units; duplicate edges, 20 sources without out-edges, a source hub.  First edge type: 21 aligned tiles with
    100 .. 120 in-edges in all (both sides of the decoder's LDS index window, wherever between them it ends), each with
    exactly one edge of its last row at the tile's last CSR position and a remainder row of ~70 edges; a hub of 112 in a
    tile's first row and one of 900 in the graph's last row.  Second edge type: its own rotation and hubs, or E = 0.
    Score kinds per row, realised through the cell's own operands (indicator features of the destination rows meeting
    entries of the score weights' rows of record slots 12 and 13): random O(1); spread over +-36 by the edge attribute
    with the row maximum on the first or on the last CSR slot; all equal (a zero input row, no score bias: u = 0);
    a common offset of +300 and of -300 with a spread of ~2.  Every value pre-activation is >= RELU_MARGIN from 0 in
    fp64 (resampled); the last six output channels are a hundred times smaller than the others; everything is far inside
    fp16's range."""
    if be is None:
        from emulator import TorchEmulatorBackend
        be = TorchEmulatorBackend()
    G = 4 if kind == "dec" else 3
    rs = np.random.RandomState(seed)
    F = F_DST
    K = (96 if kind == "dec" else 0) + F + 1
    xo = 96 if kind == "dec" else 0                           # column of x_0 in the cell's input row [h | x | 1]
    u = lambda lo, hi, *shape: rs.uniform(lo, hi, shape)
    tiny = n_dst < 16
    # ---- destination rows ----
    rkind = np.arange(n_dst) % 6
    deg0, named0 = _degrees(n_dst, 0)
    if not tiny:
        rkind[named0["hub900"]] = 2                           # the maximum in the hub's last unit
        rkind[named0["hub112"]] = 1
        for t, r in enumerate(named0["remainder"]):
            rkind[r] = (2, 1, 4, 5, 0, 3)[t % 6]
    xd = np.zeros((n_dst, F))
    xd[:, FREE_COLS] = u(0, 1, n_dst, len(FREE_COLS))
    xd[:, COL_WIDE] = (rkind == 1) | (rkind == 2)
    xd[:, COL_UP], xd[:, COL_DOWN] = rkind == 4, rkind == 5
    xd[rkind == 3] = 0.0
    xd = xd.astype(np.float32)
    T32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    P = {"x_dst": T32(xd), "sweeps": [], "meta": {"kind": rkind, "deg": [], "named": [], "n_dst": n_dst}}
    if kind == "dec":
        h_dst = u(-1, 1, n_dst, C)
        h_dst[rkind == 3] = 0.0
        P["h_dst"], P["c_in"] = T32(h_dst), T32(u(-1, 1, n_dst, C))
    skip = u(-0.15, 0.15, G, C, K) if kind == "dec" else u(-0.5, 0.5, G, C, K)
    small = np.where(np.arange(C) >= C - SMALL_CHANNELS, 0.01, 1.0)   # output channels of small magnitude
    skip *= small[None, :, None]
    if kind == "dec":
        P["c_in"] = P["c_in"] * T32(small)[None]
    P["skip"] = [T32(skip[g]) for g in range(G)]
    # ---- incoming edge types ----
    f_src = ((11, 8) if kind == "dec" else (12, 8)) if n_in == 2 else (11,)
    for d in range(n_in):
        Fs = f_src[d]
        n_src = (180, 150)[d] if not tiny else (9, 7)[d]
        idle = 20 if not tiny else 2                          # the last sources: no out-edge
        deg, named = _degrees(n_dst, d)
        if d == 1 and empty_second:
            deg, named = np.zeros(n_dst, np.int64), {"remainder": []}
        E = int(deg.sum())
        dst = np.repeat(np.arange(n_dst), deg)
        src = rs.randint(0, n_src - idle, size=E)
        if E:
            src[rs.choice(E, E // 20, replace=False)] = 3       # source hub
            first = np.concatenate([[0], np.cumsum(deg)])[:-1]
            dup = first[(deg >= 2) & (np.arange(n_dst) % 4 == 0)]
            src[dup + 1] = src[dup]                             # duplicate edges
        perm = rs.permutation(E)                                # edge ids shuffled: the CSR's perm is not the identity
        src, dst = src[perm], dst[perm]
        order = np.lexsort((np.arange(E), dst))                 # CSR order: by destination, then by edge id
        starts = np.concatenate([[0], np.cumsum(deg)])
        # the single edge at a window tile's last CSR position comes from another source than the entry in front of it
        for r in ([16 * t + 15 for t in range(WINDOW_TILES)] if d == 0 and not tiny else []):
            e_last, e_prev = order[starts[r]], order[starts[r] - 1]
            if src[e_last] == src[e_prev]:
                src[e_last] = (src[e_last] + 1) % (n_src - idle)
        slot = np.empty(E, np.int64)
        slot[order] = np.arange(E) - starts[dst[order]]
        ea = u(0.01, 0.09, E)
        ea[(rkind[dst] == 1) & (slot == 0)] = 0.1
        ea[(rkind[dst] == 2) & (slot == deg[dst] - 1)] = 0.1
        ea = ea.astype(np.float32)
        xs = u(0, 1, n_src, Fs).astype(np.float32)
        # score weights: rows 12 / 13 of the record slots carry the row kinds through the indicator columns
        score = np.zeros((G, 112 if kind == "dec" else 16, K))
        r4 = 96 if kind == "dec" else 0                        # first u4 row
        for g in range(G):
            W = score[g]
            if kind == "dec":
                W[:96, :96] = u(-0.03, 0.03, 96, 96)
                W[:96, [xo + c for c in FREE_COLS]] = u(-0.05, 0.05, 96, len(FREE_COLS))
                W[96:110, :96] = u(-0.02, 0.02, 14, 96)
                W[96:110, [xo + c for c in FREE_COLS]] = u(-0.3, 0.3, 14, len(FREE_COLS))
            else:
                W[:14, list(FREE_COLS)] = u(-1, 1, 14, len(FREE_COLS))
                if Fs <= 11:
                    W[11] = 0.0                                  # the slot that holds 1 for the value bias
            A = WIDE_A - 40.0 * g
            W[r4 + 13, xo + COL_WIDE], W[r4 + 12, xo + COL_WIDE] = A, -0.055 * A   # centred: scores about +-36
            W[r4 + 12, xo + COL_UP], W[r4 + 12, xo + COL_DOWN] = OFFSET, -OFFSET
            W[r4 + 13, xo + COL_UP] = W[r4 + 13, xo + COL_DOWN] = OFFSET_SPREAD
        sw = {"ei": torch.from_numpy(np.stack([src, dst]).astype(np.int64)).to(dev), "ea": T32(ea), "xs": T32(xs),
              "n_src": n_src, "score": [T32(score[g]) for g in range(G)],
              "l2": [T32(u(-0.2, 0.2, C, C) * small[:, None]) for _ in range(G)],
              "b_l2": [T32(u(-0.2, 0.2, C) * small) for _ in range(G)], "w_edge": [T32(u(-2, 2, C) * small) for _ in range(G)]}
        x4 = _x4_64(xs, xd, src, dst, ea, Fs)
        if kind == "dec":
            sw["h_src"] = T32(u(-1, 1, n_src, C))
            v_src = u(-1, 1, n_src, 384 * (d + 1) + 96)         # value rows at a column offset, padded rows
            ep = u(-0.1, 0.1, 4, 3, C).astype(np.float32)
            V = v_src[:, 384 * d:384 * (d + 1)].astype(np.float32).reshape(n_src, G, C)
            for _ in range(500):                               # relu margin: resample V[j, g, c] (as gc.sweep_problem)
                pre = V[src].astype(np.float64) + np.einsum("ek,gkc->egc", x4[:, :3], ep.astype(np.float64))
                close = np.zeros((n_src, G, C), bool)
                np.logical_or.at(close, src, np.abs(pre) < 1.01 * gc.RELU_MARGIN)
                if not close.any():
                    break
                V[close] = u(-1, 1, int(close.sum()))
            else:
                raise AssertionError("relu margin: no valid draw")
            v_src[:, 384 * d:384 * (d + 1)] = V.reshape(n_src, G * C)
            sw["v_src"], sw["v_off"], sw["ep"] = T32(v_src), 384 * d, T32(ep)
        else:
            # value weights: a bias of 0.6 .. 1.4 of either sign against a product of ~0.4 -- the relu is on for some edges
            # and off for others of every channel, and few pre-activations come near 0; those that do: the source's
            # features are drawn again
            value = np.zeros((G, C, 16))
            value[:, :, :Fs] = u(-0.4, 0.4, G, C, Fs)
            value[:, :, 12] = u(0.6, 1.4, G, C) * rs.choice([-1.0, 1.0], (G, C))
            value = value.astype(np.float32)
            for _ in range(2000):
                pre = np.einsum("ek,gck->egc", x4, value.astype(np.float64))
                bad = np.unique(src[(np.abs(pre) < 1.01 * gc.RELU_MARGIN).any((1, 2))])
                if bad.size == 0:
                    break
                xs[bad, 3:] = u(0, 1, bad.size, Fs - 3)
                x4 = _x4_64(xs, xd, src, dst, ea, Fs)
            else:
                raise AssertionError("relu margin: no valid draw")
            sw["xs"], sw["value"] = T32(xs), [T32(value[g]) for g in range(G)]
        P["sweeps"].append(sw)
        P["meta"]["deg"].append(deg)
        P["meta"]["named"].append(named)
    return attach_csr(P, be)


def attach_csr(P, be, csrs=None):
    """P with the CSR tables (`csrs`, or freshly built by `be` from every sweep's edge list) and the edge records of
    ggnn_edge_prepare on them.  Returns P (a shallow copy when `csrs` is given)."""
    if csrs is not None:
        P = dict(P, sweeps=[dict(sw) for sw in P["sweeps"]])
    n_dst, dev = P["x_dst"].size(0), P["x_dst"].device
    for d, sw in enumerate(P["sweeps"]):
        csr = be.build_csr(sw["ei"], sw["n_src"], n_dst) if csrs is None else csrs[d]
        E = sw["ei"].size(1)
        einfo = torch.zeros(E + 3, 20, device=dev)
        be.edge_prepare([(csr, sw["ea"], sw["xs"], P["x_dst"], einfo)])
        sw.update(csr=csr, rowptr=csr.rowptr[:n_dst + 1], col=csr.col, einfo=einfo)
    return P


def value_preactivations(kind, P):
    """Every V + W3 r (dec) / W_value x~ + b (enc) of the problem in fp64, from the edge records: [sum E, G, 96]."""
    D = torch.float64
    t = lambda v: v.detach().cpu().to(D)
    G = 4 if kind == "dec" else 3
    out = []
    for sw in P["sweeps"]:
        E = int(sw["rowptr"][-1])
        src, einfo = sw["col"].cpu().long()[:E], t(sw["einfo"])
        for g in range(G):
            if kind == "dec":
                out.append(t(sw["v_src"])[src][:, sw["v_off"] + g * C: sw["v_off"] + (g + 1) * C] + einfo[:E, 16:19] @ t(sw["ep"])[g])
            else:
                out.append(einfo[:E, :16] @ t(sw["value"][g]).t())
    return torch.cat(out) if out else torch.zeros(0, C, dtype=D)


# --------------------------------------------------------------------------------------------------------------------
# Per-element magnitudes of (h, c)
# --------------------------------------------------------------------------------------------------------------------
# sigmoid and tanh are read out on the hardware exp / rcp units (csrc/common.h): an ABSOLUTE error of up to ~3e-7 on
# outputs in [-1, 1], whatever the size of the result (tanh(x) = 1 - 2 rcp(1 + exp(2x)) for a small x)
READOUT_FLOOR = 3e-7
ROUND_FP32 = 2e-7    # three fp32 roundings (two products, one sum) of the update itself


def _dsig(z, delta):
    """max of sigmoid' over [z - delta, z + delta] (sigmoid' falls with |z|)."""
    s = torch.sigmoid((z.abs() - delta).clamp(min=0))
    return s * (1 - s)


def _dtanh(z, delta):
    return 1 - torch.tanh((z.abs() - delta).clamp(min=0)) ** 2


def cell_magnitudes(kind, P, tol=gc.SWEEP_TOL):
    """{"h", "c"}: per-element magnitudes [n_dst, 96] in units of `tol` (|got - ref64| <= tol * magnitude passes), and
    "z": the gate pre-activations' own.

    A gate pre-activation z_g is a sum; its magnitude is the sum of its terms' magnitudes:
      sum |x| |w| of the skip product (input row [h | x | 1]),
      per edge type sum_c |l2[o, c]| M_A[c]  +  |b_l2| sum alpha  +  |w_edge| sum alpha a (1 + KAPPA_W kappa),
    with the aggregate's magnitude M_A = sum alpha |val| (1 + KAPPA_W kappa): alpha carries the relative error gradcheck
    derives (fp32 scores are off by a few eps kappa, kappa = the row's largest sum |u| |x| score magnitude; __expf by eps
    |s - max|).  sum alpha a weights DIFFERENT a_e with those alphas, so it carries the factor like the aggregate does.
    sum alpha does not: every alpha_e is p_e over the same den, their sum is den / (den + 1e-16) whatever the errors of the
    p_e, so as a term of z_g it is exact to a rounding.  (gradcheck.forward_excess, which grades the sweep's own sum alpha
    column, keeps the factor there: that bound is the one its issue states, and it contains this one.)
    An error delta_g = tol m_g of z_g moves c and h by at most |dc/dz_g| delta_g: the derivatives of the LSTM update, each
    taken at its largest over [z_g - delta_g, z_g + delta_g] so that the bound also holds where a gate saturates, plus the
    product of the two first-order terms of i tanh(c~).  On top: READOUT_FLOOR per sigmoid / tanh read-out and the update's
    own fp32 roundings."""
    D = torch.float64
    t = lambda v: v.detach().cpu().to(D)
    x, n = t(P["x_dst"]), P["x_dst"].size(0)
    G = 4 if kind == "dec" else 3
    ones = torch.ones(n, 1, dtype=D)
    xin = torch.cat([t(P["h_dst"]), x, ones], 1) if kind == "dec" else torch.cat([x, ones], 1)
    z, m = [], []
    for g in range(G):
        W = t(P["skip"][g])
        zg, mg = xin @ W.t(), xin.abs() @ W.abs().t()
        for sw in P["sweeps"]:
            rowptr = sw["rowptr"].cpu().long()
            E = int(rowptr[-1])
            dst = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
            src, einfo = sw["col"].cpu().long()[:E], t(sw["einfo"])
            x4, reloc, a = einfo[:E, :16], einfo[:E, 16:19], einfo[:E, 19]
            u = xin @ t(sw["score"][g]).t()
            if kind == "dec":
                hs = t(sw["h_src"])[src]
                sc = (u[dst, :96] * hs).sum(-1) + (u[dst, 96:] * x4).sum(-1)
                kap = (u[dst, :96].abs() * hs.abs()).sum(-1) + (u[dst, 96:].abs() * x4.abs()).sum(-1)
                val = torch.relu(t(sw["v_src"])[src][:, sw["v_off"] + g * C: sw["v_off"] + (g + 1) * C] + reloc @ t(sw["ep"])[g])
            else:
                sc = (u[dst] * x4).sum(-1)
                kap = (u[dst].abs() * x4.abs()).sum(-1)
                val = torch.relu(x4 @ t(sw["value"][g]).t())
            kappa = torch.zeros(n, dtype=D).scatter_reduce(0, dst, kap, "amax")
            smax = torch.full((n,), float("-inf"), dtype=D).scatter_reduce(0, dst, sc, "amax")
            p = (sc - smax[dst]).exp()
            den = torch.zeros(n, dtype=D).index_add(0, dst, p)
            alpha = p / (den[dst] + 1e-16)
            fac = 1 + gc.KAPPA_W * kappa
            A = torch.zeros(n, C, dtype=D).index_add(0, dst, alpha[:, None] * val)
            sa = torch.zeros(n, dtype=D).index_add(0, dst, alpha)
            sae = torch.zeros(n, dtype=D).index_add(0, dst, alpha * a)
            l2, b, we = t(sw["l2"][g]), t(sw["b_l2"][g]), t(sw["w_edge"][g])
            zg = zg + A @ l2.t() + sa[:, None] * b[None] + sae[:, None] * we[None]
            mg = mg + (A * fac[:, None]) @ l2.abs().t() + sa[:, None] * b.abs()[None] + (sae.abs() * fac)[:, None] * we.abs()[None]
        z.append(zg)
        m.append(mg)
    dl = [tol * v for v in m]
    gi, gt, go = (0, 2, 3) if kind == "dec" else (0, 1, 2)
    i, tt_, o = torch.sigmoid(z[gi]), torch.tanh(z[gt]), torch.sigmoid(z[go])
    di, dt_ = _dsig(z[gi], dl[gi]) * m[gi], _dtanh(z[gt], dl[gt]) * m[gt]
    c = i * tt_
    mc = tt_.abs() * di + i * dt_ + tol * di * dt_
    floor_c = READOUT_FLOOR * 2 + ROUND_FP32 * c.abs()
    if kind == "dec":
        c_in, f = t(P["c_in"]), torch.sigmoid(z[1])
        c = c + f * c_in
        mc = mc + c_in.abs() * _dsig(z[1], dl[1]) * m[1]
        floor_c = READOUT_FLOOR * (c_in.abs() + 2) + ROUND_FP32 * ((f * c_in).abs() + (i * tt_).abs())
    mc = mc + floor_c / tol
    h = o * torch.tanh(c)
    dc = _dtanh(c, tol * mc) * mc
    mh = torch.tanh(c).abs() * _dsig(z[go], dl[go]) * m[go] + o * dc + tol * _dsig(z[go], dl[go]) * m[go] * dc \
        + (READOUT_FLOOR * 2 + ROUND_FP32 * h.abs()) / tol
    return {"h": mh, "c": mc, "z": m}


def cell_excess(got, ref, mag, tol=gc.SWEEP_TOL):
    """The worst |got - ref| / (tol * magnitude) over every element of (h, c), and where: (ratio, (name, row, channel)).
    A non-finite element of `got` is an infinite ratio."""
    worst = (0.0, None)
    for name, a, b in zip(("h", "c"), got, ref):
        a = a.detach().cpu().double()
        bad = ~torch.isfinite(a)
        if bool(bad.any()):
            return float("inf"), (name,) + tuple(int(v) for v in torch.nonzero(bad)[0])
        r, idx = gc.bound_excess(a, b, mag[name], tol)
        if r > worst[0]:
            worst = (r, (name,) + tuple(int(v) for v in idx))
    return worst
