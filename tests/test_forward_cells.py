"""The fused forward cells (ggnn_decoder_cell_batch, ggnn_encoder_cell_batch) against an fp64 restatement of the cell
from the original fp32 weights, element by element, on problems built at the sweep's edges (tests/cellcheck.py); the split
plan, the block-major value rows and CSR tables refilled in place on the same problems.  The CPU tests at the end show
that the check accepts the torch emulator and the fp32 restatement and sees one-term bugs, each by name.
"""
import functools

import numpy as np
import pytest
import torch

import cellcheck as cc
import gradcheck as gc
from emulator import TorchEmulatorBackend

# (kind, n_in, second edge type empty, n_dst)
CASES = [(kind, n_in, empty, n_dst) for kind in ("dec", "enc")
         for n_in, empty, n_dst in ((2, False, cc.N_DST), (2, True, cc.N_DST), (1, False, cc.N_DST), (2, False, cc.N_TINY))]
MAIN = {kind: (kind, 2, False, cc.N_DST) for kind in ("dec", "enc")}


def _case_id(case):
    kind, n_in, empty, n_dst = case
    return f"{kind}-n_in{n_in}" + ("-second_empty" if empty else "") + f"-n_dst{n_dst}"


def backend():
    from graingraphnn_amd.backend import default_backend
    return default_backend()


@functools.lru_cache(maxsize=None)
def _case(case, dev="cpu"):
    """(P, fp64 reference (h, c), magnitudes) of a case, computed once and shared: nobody changes them."""
    kind, n_in, empty, n_dst = case
    be = backend() if dev == "cuda" else TorchEmulatorBackend()
    P = cc.cell_problem(kind, 100 + CASES.index(case), n_in, n_dst, empty, be, dev)
    pre = cc.value_preactivations(kind, P)
    assert pre.numel() == 0 or float(pre.abs().min()) >= gc.RELU_MARGIN, "a value pre-activation is too near 0"
    for t in [P["x_dst"]] + [s[k] for s in P["sweeps"] for k in ("einfo", "xs")] + [w for s in P["sweeps"] for w in s["score"]]:
        assert float(t.abs().max()) < 65504.0
    return P, cc._cell_reference(kind, P, torch.float64), cc.cell_magnitudes(kind, P)


def _run(be, kind, P):
    """(h, c) of the fused cell of `be` on P (clones), and the call tuple."""
    call, _ = cc._rebuild_wide_call(be, kind, P)
    (be.decoder_cell_batch if kind == "dec" else be.encoder_cell_batch)([call])
    return (call[-2].clone(), call[-1].clone()), call


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
@torch.no_grad()
def test_fused_cell_against_fp64_per_element(case):
    """h and c of the fused cell within the per-element bound of the fp64 restatement everywhere: degrees 0-7 with
    unequal pairs in flight, hubs of 112 and 900, tiles of 100 .. 120 in-edges around the LDS index window with one edge at
    the tile's last CSR position, a slid-back last tile, n_dst = 5; scores over +-36 with the maximum in the first or the
    last unit, all-equal rows, offsets of +-300; one and two incoming edge types, one of them empty.  Bit-reproducible,
    range flag clear."""
    kind = case[0]
    be = backend()
    P, ref, mag = _case(case, "cuda")
    be.range_exceeded("cuda")                      # clear
    got, call = _run(be, kind, P)
    call[-2].fill_(float("nan")), call[-1].fill_(float("nan"))
    (be.decoder_cell_batch if kind == "dec" else be.encoder_cell_batch)([call])
    assert torch.equal(call[-2], got[0]) and torch.equal(call[-1], got[1])      # no atomics: bit-reproducible
    assert not be.range_exceeded("cuda")
    r, idx = cc.cell_excess(got, ref, mag)
    r32, _ = cc.cell_excess(cc._cell_reference(kind, P, torch.float32), ref, mag)
    E = [int(sw["ei"].size(1)) for sw in P["sweeps"]]
    print(f"{_case_id(case)} E={E}: worst |hip - ref64| / bound {r:.3f} at {idx} (fp32 restatement: {r32:.3f})")
    assert r <= 1.0, (case, r, idx)


def _split_plan(be, P):
    """The decoder cell of P as projection + ggnn_period_gat_aggregate_batch + ggnn_lstm_epilogue (the split plan's
    kernels, called directly): (h, c)."""
    from graingraphnn_amd import _lib
    from graingraphnn_amd.packing import bf16_planes
    dev = P["x_dst"].device
    n, F = P["x_dst"].shape
    G, n_in, Fp = 4, len(P["sweeps"]), (F + 3) & ~3
    u_off = [d * G * 112 for d in range(n_in)]                 # per edge type: u_h (G x 96) then u4 (G x 16)
    s_off = n_in * G * 112
    ncols = (s_off + G * 96 + 95) // 96 * 96
    Wall = torch.zeros(ncols, 96 + F + 1, device=dev)          # rows over the cell's input [h | x | 1]
    for d, sw in enumerate(P["sweeps"]):
        for g in range(G):
            Wall[u_off[d] + 96 * g: u_off[d] + 96 * (g + 1)] = sw["score"][g][:96]
            Wall[u_off[d] + 96 * G + 16 * g: u_off[d] + 96 * G + 16 * (g + 1)] = sw["score"][g][96:]
    for g in range(G):
        Wall[s_off + 96 * g: s_off + 96 * (g + 1)] = P["skip"][g]
    wp = torch.zeros(ncols, Fp + 96, device=dev)
    wp[:, :F], wp[:, Fp:], bp = Wall[:, 96:96 + F], Wall[:, :96], Wall[:, 96 + F].contiguous()
    p_dst = torch.empty(n, ncols, device=dev)
    be.project_batch([(P["x_dst"], F, P["h_dst"], wp, bp, p_dst)])
    Ka = 96 * n_in + 4
    Kg = (Ka + 31) // 32 * 32
    agg = torch.zeros(n, G * Kg, device=dev)
    w2 = torch.zeros(G, 96, Ka, device=dev)
    sweeps = []
    for d, sw in enumerate(P["sweeps"]):
        for g in range(G):
            w2[g, :, 96 * d:96 * (d + 1)] = sw["l2"][g]
            w2[g, :, 96 * n_in + 2 * d], w2[g, :, 96 * n_in + 2 * d + 1] = sw["b_l2"][g], sw["w_edge"][g]
        sweeps.append((sw["csr"], sw["einfo"], sw["v_src"], p_dst, sw["h_src"], sw["ep"], agg, sw["v_off"], u_off[d],
                       u_off[d] + 96 * G, 96 * d, Kg, 96 * n_in + 2 * d, G))
    be.aggregate_batch(sweeps)
    h, c = torch.empty(n, 96, device=dev), torch.empty(n, 96, device=dev)
    be.lstm_epilogue(agg, w2, p_dst, s_off, P["c_in"], h, c, None, G, _lib.MODE_LSTM, bf16_planes(w2), Kg)
    return h, c


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "dec"], ids=_case_id)
@torch.no_grad()
def test_split_plan_against_fp64_per_element(case):
    """The same decoder problems through the split plan's kernels -- the fall-back for weights beyond the fused cell's
    range -- held to the same bound."""
    P, ref, mag = _case(case, "cuda")
    got = _split_plan(backend(), P)
    r, idx = cc.cell_excess(got, ref, mag)
    print(f"split plan {_case_id(case)}: worst |hip - ref64| / bound {r:.3f} at {idx}")
    assert r <= 1.0, (case, r, idx)


@pytest.mark.gpu
@torch.no_grad()
def test_block_major_value_rows_on_the_edge_problem():
    """v_block_major value rows ([blocks][n_src][96]) on the edge problem: the row-major result bit for bit."""
    be = backend()
    P, _, _ = _case(MAIN["dec"], "cuda")
    want, call = _run(be, "dec", P)
    sweeps = []
    for csr, einfo, h_src, v_src, v_off, ep in call[0]:
        n, w = v_src.shape
        assert w % 96 == 0
        bm = v_src.reshape(n, w // 96, 96).permute(1, 0, 2).contiguous().view(n, w)
        sweeps.append((csr, einfo, h_src, bm, v_off, ep, True))
    call2 = (sweeps,) + tuple(call[1:6]) + (torch.full_like(call[6], float("nan")), torch.full_like(call[7], float("nan")))
    be.decoder_cell_batch([call2])
    assert torch.equal(call2[6], want[0]) and torch.equal(call2[7], want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dec", "enc"])
@torch.no_grad()
def test_cells_on_csr_tables_refilled_in_place(kind):
    """Tables carved for a larger capacity, filled with a longer list and refilled with the problem's: behind the list's
    end they hold the longer list's entries (valid indices of other nodes).  Both cells give the bits of freshly built
    tables: nothing behind a list's end is read into a result."""
    be = backend()
    P, _, _ = _case(MAIN[kind], "cuda")
    want, _ = _run(be, kind, P)
    n_dst = P["x_dst"].size(0)
    rs = np.random.RandomState(9)
    extra = 700
    tables = be.csr_in_place([(sw["ei"].size(1) + extra, sw["n_src"], n_dst) for sw in P["sweeps"]], "cuda")
    longer = []
    for sw in P["sweeps"]:
        more = np.stack([rs.randint(0, sw["n_src"], extra), rs.randint(0, n_dst, extra)]).astype(np.int64)
        longer.append(torch.cat([sw["ei"], torch.from_numpy(more).cuda()], 1).contiguous())
    tables.rebuild(longer)
    csrs = tables.rebuild([sw["ei"].contiguous() for sw in P["sweeps"]])
    for csr, sw in zip(csrs, P["sweeps"]):
        E = sw["ei"].size(1)
        assert csr.E == E and csr.col.numel() == E + extra
        assert torch.equal(csr.col[:E], sw["csr"].col[:E]) and torch.equal(csr.rowptr, sw["csr"].rowptr)
    got, _ = _run(be, kind, cc.attach_csr(P, be, csrs))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the check accepts the emulator and the fp32 restatement, and sees one-term bugs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_case_id)
@torch.no_grad()
def test_cell_check_accepts_the_emulator_and_the_fp32_restatement(case):
    """The torch emulator of the cells' contract (fp32, on the decoded weight stream) at <= 1, the torch float32
    evaluation of the restatement at <= 0.5 of the bound on every element: the tolerance is the reference's own."""
    kind = case[0]
    P, ref, mag = _case(case)
    emu = TorchEmulatorBackend()
    got, _ = _run(emu, kind, P)
    r, idx = cc.cell_excess(got, ref, mag)
    r32, idx32 = cc.cell_excess(cc._cell_reference(kind, P, torch.float32), ref, mag)
    print(f"{_case_id(case)}: emulator {r:.3f} at {idx}, fp32 restatement {r32:.3f} at {idx32}")
    assert r <= 1.0, (case, r, idx)
    assert r32 <= 0.5, (case, r32, idx32)


def _buggy_cell(kind, P, bug):
    """A copy of the restatement (cellcheck._cell_reference, float32) with one bug: "no_max" softmax without the max
    subtraction; "no_rescale" the online softmax over units of three edges whose accumulators are not rescaled when a
    later unit raises the maximum; "bias_weight_one" b_l2 added with weight 1 instead of sum alpha; "no_epsilon" the
    denominator without + 1e-16.  bug=None: the same code without a bug (the unit-wise softmax included)."""
    dtype = torch.float32
    t = lambda v: v.cpu().to(dtype)
    x, n = t(P["x_dst"]), P["x_dst"].size(0)
    G = 4 if kind == "dec" else 3
    ones = torch.ones(n, 1, dtype=dtype)
    xin = torch.cat([t(P["h_dst"]), x, ones], 1) if kind == "dec" else torch.cat([x, ones], 1)
    pre = []
    for g in range(G):
        z = xin @ t(P["skip"][g]).t()
        for sw in P["sweeps"]:
            rowptr = sw["rowptr"].cpu().long()
            E = int(rowptr[-1])
            deg = rowptr[1:] - rowptr[:-1]
            dst = torch.repeat_interleave(torch.arange(n), deg)
            slot = torch.arange(E) - rowptr[:-1][dst]
            src = sw["col"].cpu().long()[:E]
            einfo = t(sw["einfo"])
            x4, reloc, a = einfo[:E, :16], einfo[:E, 16:19], einfo[:E, 19]
            u = xin @ t(sw["score"][g]).t()
            if kind == "dec":
                sc = (u[dst, :96] * t(sw["h_src"])[src]).sum(-1) + (u[dst, 96:] * x4).sum(-1)
                val = torch.relu(t(sw["v_src"])[src][:, sw["v_off"] + g * 96: sw["v_off"] + (g + 1) * 96] + reloc @ t(sw["ep"])[g])
            else:
                sc = (u[dst] * x4).sum(-1)
                val = torch.relu(x4 @ t(sw["value"][g]).t())
            eps = 0.0 if bug == "no_epsilon" else 1e-16
            if bug == "no_max":
                p = sc.exp()
                den = torch.zeros(n, dtype=dtype).index_add(0, dst, p)
                alpha = p / (den[dst] + eps)
                A = torch.zeros(n, 96, dtype=dtype).index_add(0, dst, alpha[:, None] * val)
                sa = torch.zeros(n, dtype=dtype).index_add(0, dst, alpha)
                sae = torch.zeros(n, dtype=dtype).index_add(0, dst, alpha * a)
            else:   # unit by unit, as the kernels fold a row: running maximum, accumulators rescaled by exp(old - new)
                mx = torch.full((n,), float("-inf"), dtype=dtype)
                den, sae, A = torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype), torch.zeros(n, 96, dtype=dtype)
                for k in range(int((deg.max() + 2) // 3) if E else 0):
                    e = torch.nonzero(slot // 3 == k).reshape(-1)
                    mnew = mx.scatter_reduce(0, dst[e], sc[e], "amax")
                    scale = torch.where(torch.isfinite(mx), (mx - mnew).exp(), torch.zeros_like(mx))
                    if bug == "no_rescale":
                        scale = torch.ones_like(scale)
                    p = (sc[e] - mnew[dst[e]]).exp()
                    den = (den * scale).index_add(0, dst[e], p)
                    sae = (sae * scale).index_add(0, dst[e], p * a[e])
                    A = (A * scale[:, None]).index_add(0, dst[e], p[:, None] * val[e])
                    mx = mnew
                inv = 1.0 / (den + eps)
                A, sa, sae = A * inv[:, None], den * inv, sae * inv
            if bug == "bias_weight_one":
                sa = torch.ones_like(sa)
            z = z + A @ t(sw["l2"][g]).t() + sa[:, None] * t(sw["b_l2"][g])[None] + sae[:, None] * t(sw["w_edge"][g])[None]
        pre.append(z)
    if kind == "dec":
        c = torch.sigmoid(pre[1]) * t(P["c_in"]) + torch.sigmoid(pre[0]) * torch.tanh(pre[2])
        return torch.sigmoid(pre[3]) * torch.tanh(c), c
    c = torch.sigmoid(pre[0]) * torch.tanh(pre[1])
    return torch.sigmoid(pre[2]) * torch.tanh(c), c


def _with_edges_changed(kind, P, change):
    """P with the first edge type's CSR tables edited by `change(rowptr, col, einfo) -> (rowptr, col, einfo)` (copies)."""
    sw = dict(P["sweeps"][0])
    E = int(sw["rowptr"][-1])
    sw["rowptr"], sw["col"], sw["einfo"] = change(sw["rowptr"].clone().long(), sw["col"][:E].clone(), sw["einfo"].clone())
    return dict(P, sweeps=[sw] + list(P["sweeps"][1:]))


# DC_CW of csrc/dec_cell.hip (source indices of a tile kept in LDS; the window variant runs up to DC_CW - 2 in-edges).  The
# value only SELECTS the tile bug (d) is injected into: any of the tiles with 100 .. 120 in-edges has one edge at its last
# CSR position, so the injection stays valid if the kernel's constant moves
WINDOW_SIZE = 111


@pytest.mark.parametrize("kind", ["dec", "enc"])
@torch.no_grad()
def test_cell_check_sees_one_term_bugs(kind):
    """Each of the bugs a plausible edit of the cells makes is rejected (ratio > 1 or a non-finite value); the same code
    without the bug is accepted."""
    P, ref, mag = _case(MAIN[kind])
    worst = lambda got: cc.cell_excess(got, ref, mag)[0]
    good = cc._cell_reference(kind, P, torch.float32)
    assert worst(_buggy_cell(kind, P, None)) <= 0.5
    n, deg = P["x_dst"].size(0), torch.from_numpy(P["meta"]["deg"][0])
    assert int((deg == 0).sum()) > 10
    # (a) softmax without the max subtraction: the rows with a common offset overflow (inf / inf) or underflow (0 / 1e-16)
    assert worst(_buggy_cell(kind, P, "no_max")) > 1.0
    # (b) the accumulators not rescaled when a later unit raises the maximum (rows whose maximum is on the last slot)
    assert worst(_buggy_cell(kind, P, "no_rescale")) > 1.0
    # (c) the last edge of a row dropped when degree = 1 (mod 3)
    def drop(rowptr, col, einfo):
        d = rowptr[1:] - rowptr[:-1]
        keep = torch.ones(col.numel(), dtype=torch.bool)
        keep[(rowptr[1:] - 1)[d % 3 == 1]] = False
        d = d - (d % 3 == 1).long()
        return (torch.cat([torch.zeros(1, dtype=torch.long), d.cumsum(0)]), col[keep],
                torch.cat([einfo[:col.numel()][keep], torch.zeros(3, 20)]))
    assert worst(cc._cell_reference(kind, _with_edges_changed(kind, P, drop), torch.float32)) > 1.0
    # (d) in the tile with as many in-edges as the window holds, the last edge's source replaced by the previous entry
    def previous(rowptr, col, einfo):
        t = WINDOW_SIZE - cc.WINDOW_LO
        assert int(rowptr[16 * t + 16] - rowptr[16 * t]) == WINDOW_SIZE and int(rowptr[16 * t + 16] - rowptr[16 * t + 15]) == 1
        p = int(rowptr[16 * t + 16]) - 1
        assert int(col[p]) != int(col[p - 1])
        col[p] = col[p - 1]
        if kind == "enc":                           # (the encoder cell reads the source's features from the edge record)
            einfo[p] = einfo[p - 1]
        return rowptr, col, einfo
    assert worst(cc._cell_reference(kind, _with_edges_changed(kind, P, previous), torch.float32)) > 1.0
    # (e) b_l2 added with weight 1 instead of sum alpha (rows without in-edges), (f) the + 1e-16 missing (0 / 0 there)
    assert worst(_buggy_cell(kind, P, "bias_weight_one")) > 1.0
    assert worst(_buggy_cell(kind, P, "no_epsilon")) == float("inf")
    # (g) the last n_dst % 16 rows taken from rows shifted by one
    k = n % 16
    assert k > 0
    bad = [v.clone() for v in good]
    for v in bad:
        v[n - k:] = v[n - k - 1:n - 1].clone()
    assert worst(bad) > 1.0
    # (h) one small output element moved by 3 x its own bound: invisible to a max-norm criterion (the one of
    # test_fused_cells_are_fp32_equivalent_on_wide_range_operands), which is why the bound is per element
    idx = np.unravel_index(int(torch.argmin(mag["c"])), mag["c"].shape)
    bad = [v.clone() for v in good]
    bad[1][idx] += 3 * gc.SWEEP_TOL * float(mag["c"][idx])
    assert worst(bad) > 1.0
    scale = float(ref[1].abs().max())
    e_f32 = float((good[1].double() - ref[1]).abs().max()) / scale
    e_bad = float((bad[1].double() - ref[1]).abs().max()) / scale
    assert e_bad <= 2.0 * e_f32 + 5e-7 and e_bad < 1e-5


@pytest.mark.parametrize("kind", ["dec", "enc"])
@torch.no_grad()
def test_cell_problem_is_what_it_says(kind):
    """The structure of the edge problem: totals of the window tiles, one edge at their last position, hubs where they
    belong in both edge types, every score kind on rows of no, one and several units, and -- for every gate of both edge
    types, through the cell's own operands -- the scores the kinds promise."""
    P, _, _ = _case(MAIN[kind])
    n = P["x_dst"].size(0)
    assert n == cc.N_DST and n % 16 and 2 * 128 < n <= 3 * 128
    rp = P["sweeps"][0]["rowptr"].long()
    deg = rp[1:] - rp[:-1]
    assert torch.equal(deg, torch.from_numpy(P["meta"]["deg"][0]))
    tiles = (rp[16:16 * cc.WINDOW_TILES + 1:16] - rp[0:16 * cc.WINDOW_TILES:16]).tolist()
    assert tiles == list(range(100, 121))
    assert all(int(deg[16 * t + 15]) == 1 for t in range(cc.WINDOW_TILES))
    assert int(deg[16 * cc.WINDOW_TILES]) == 112 and int(deg[n - 1]) == 900
    kinds = P["meta"]["kind"]
    for k in range(len(cc.KINDS)):
        units = set(((deg[torch.from_numpy(kinds == k)] + 2) // 3).tolist())
        assert {0, 1, 2, 3} <= units, (cc.KINDS[k], units)
    ei = P["sweeps"][0]["ei"]
    pairs = ei[0] * n + ei[1]
    assert pairs.unique().numel() < pairs.numel()                                   # duplicate edges
    assert int(ei[0].max()) < P["sweeps"][0]["n_src"] - 20                          # sources without out-edges
    assert int(torch.bincount(ei[0]).max()) > 100                                   # a source hub
    t = lambda v: v.double()
    ones = torch.ones(n, 1, dtype=torch.float64)
    xin = torch.cat(([t(P["h_dst"])] if kind == "dec" else []) + [t(P["x_dst"]), ones], 1)
    for d, sw in enumerate(P["sweeps"]):
        rp = sw["rowptr"].long()
        deg = rp[1:] - rp[:-1]
        named = P["meta"]["named"][d]
        assert int(deg[named["hub112"]]) == 112 and int(deg[named["hub900"]]) == 900
        hub = named["hub900"]
        assert kinds[hub] == 2                                                      # wide, the maximum on its last slot
        E = int(rp[-1])
        dst = torch.repeat_interleave(torch.arange(n), deg)
        k = torch.from_numpy(kinds)[dst]
        x4 = t(sw["einfo"])[:E, :16]
        for g in range(len(sw["score"])):
            u = xin @ t(sw["score"][g]).t()
            if kind == "dec":
                sc = (u[dst, :96] * t(sw["h_src"])[sw["col"].long()[:E]]).sum(-1) + (u[dst, 96:] * x4).sum(-1)
            else:
                sc = (u[dst] * x4).sum(-1)
            s = sc[int(rp[hub]):int(rp[hub + 1])]
            assert int(torch.argmax(s)) == s.numel() - 1 and float(s.max() - s.min()) > 50, (d, g)   # ... in the last unit
            r1 = int(torch.nonzero((torch.from_numpy(kinds) == 1) & (deg == 7))[0])
            s = sc[int(rp[r1]):int(rp[r1 + 1])]
            assert int(torch.argmax(s)) == 0 and float(s.max() - s.min()) > 50, (d, g)
            assert float(sc[k == 4].min()) > 250 and float(sc[k == 5].max()) < -250, (d, g)
            assert float(sc[k == 3].abs().max()) == 0.0, (d, g)
