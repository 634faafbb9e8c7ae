"""Shared checking code of the training backward: fp64 restatements of the sweep and of the heads with per-element
error magnitudes, the sweep test problem, and the relu-kink rule of the gradient fuzz.

Bounds are per element, against the fp64 magnitude of that element's own sum (never against a tensor's largest entry):
a row whose gradient is 1 % of the tensor's largest is held to its own size.
"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

C = 96
JJ = ("joint", "connect", "joint")

# --------------------------------------------------------------------------------------------------------------------
# The sweep (ggnn_period_gat_aggregate) and its backward
# --------------------------------------------------------------------------------------------------------------------
SWEEP_TOL = 2e-5
# fp32 scores carry an absolute rounding of a few eps * kappa (kappa = sum |u| |x| of the row's scores) and __expf a
# relative one of eps * |s - max|: alpha is off by <= ~1e-6 kappa relative, i.e. 0.05 kappa in units of SWEEP_TOL
KAPPA_W = 0.05
RELU_MARGIN = 1e-3   # every V + W3 r of a sweep problem is at least this far from 0: no relu tie in the reference
OUTPUTS = ("g_p_dst", "g_p_src", "g_h_src", "g_ep")


def sweep_layout(G, et, lay_src, lay_dst):
    """The sweep's column offsets as training.py passes them, from train_pack.packed_weights' layout."""
    return dict(v_off=lay_src.v_off[et], u_off=lay_dst.u_off.get(et, 0), u4_off=lay_dst.u4_off[et],
                a_off=lay_dst.a_off[et], a_gstride=lay_dst.Kg, sc_off=lay_dst.sc_off[et], G=G,
                ldp_src=lay_src.ncols, ldp_dst=lay_dst.ncols, ld_agg=G * lay_dst.Kg)


def offsets(L):
    return (L["v_off"], L["u_off"], L["u4_off"], L["a_off"], L["a_gstride"], L["sc_off"], L["G"])


def training_layouts():
    """(encoder layout, decoder layout) {node type: NodeLayout} of the default model's cells."""
    from graingraphnn_amd import synthetic, train_pack
    from graingraphnn_amd.models import GrainNN_regressor
    R = GrainNN_regressor(synthetic.default_hyper("cpu"))
    out = []
    for cell, gates, sees_h in ((R.gclstm_encoder.cell_list[0], "ico", False), (R.gclstm_decoder.cell_list[0], "ifco", True)):
        out.append(train_pack.packed_weights(cell, gates, cell.in_channels_dict, sees_h)[0])
    return out


def _amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def min_image(xs, xd):
    rel = xs - xd
    return torch.where(rel > 0.5, -1.0, torch.where(rel < -0.5, 1.0, 0.0)).to(rel.dtype) + rel


def sweep_problem(L, has_h, seed, n_src=1500, n_dst=3251, Fs=11, Fd=8, empty=False):
    """A sweep problem at its edges (CPU tensors).  Destination rows of degree 0, 1, 2, 3, 4, 6, 7 (one and several
    units of GGNN_UNIT_EDGES = 3), hubs of 900 and 3000 in-edges, duplicate edges, 20 sources without out-edges and a
    source hub of 500; n_dst > 3072 waves of the destination pass and not a multiple of 4.  Score kinds per row: random,
    spread over +-36 by the edge attribute with the row maximum on the first or on the last CSR slot (the last unit: the
    online max rescale), all equal (u = 0).  Every V + W3 r is >= RELU_MARGIN away from 0 (resampled).  `empty`: E = 0."""
    G = L["G"]
    rs = np.random.RandomState(seed)
    deg = np.array([0, 1, 2, 3, 4, 6, 7])[np.arange(n_dst) % 7]
    if empty:
        deg[:] = 0
    else:
        deg[5], deg[11], deg[n_dst - 2] = 900, 3000, 900
    E = int(deg.sum())
    dst = np.repeat(np.arange(n_dst), deg)
    src = rs.randint(0, n_src - 20, size=E)                    # the last 20 sources: no out-edge
    if E:
        src[rs.choice(E, 500, replace=False)] = 3              # source hub
    perm = rs.permutation(E)                                   # edge ids shuffled: the CSR's perm is not the identity
    src, dst = src[perm], dst[perm]
    order = np.lexsort((np.arange(E), dst))                    # CSR order: by destination, then by edge id
    slot_in_row = np.empty(E, np.int64)
    starts = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n_dst))])
    slot_in_row[order] = np.arange(E) - starts[dst[order]]
    kind = np.arange(n_dst) % 5                                 # 0 random, 1 wide max-first, 2 wide max-last, 3 equal, 4 wide
    if not empty:
        kind[11] = 2                                           # the 3000-hub: wide, maximum in its last unit
        kind[5] = 0
    ea = rs.uniform(0.01, 0.09, E)
    first, last = slot_in_row == 0, slot_in_row == deg[dst] - 1
    ea[(kind[dst] == 1) & first] = 0.1
    ea[(kind[dst] == 2) & last] = 0.1
    ea = ea.astype(np.float32)
    xs = rs.uniform(0, 1, (n_src, Fs)).astype(np.float32)
    xd = rs.uniform(0, 1, (n_dst, Fd)).astype(np.float32)
    p_src = rs.uniform(-50, 50, (n_src, L["ldp_src"])).astype(np.float32)    # columns the sweep must not read: junk
    p_dst = rs.uniform(-50, 50, (n_dst, L["ldp_dst"])).astype(np.float32)
    for g in range(G):
        u4 = rs.uniform(-0.5, 0.5, (n_dst, 16))
        A = np.where(kind == 4, rs.uniform(-400, 400, n_dst), 800.0)
        wide = (kind == 1) | (kind == 2) | (kind == 4)
        u4[wide, 13] = A[wide]
        u4[wide, 12] = -0.055 * A[wide]                         # centres the spread: scores about +-36
        u4[kind == 3] = 0.0
        p_dst[:, L["u4_off"] + 16 * g:L["u4_off"] + 16 * (g + 1)] = u4
        if has_h:
            uh = rs.uniform(-0.3, 0.3, (n_dst, C))
            uh[kind == 3] = 0.0
            p_dst[:, L["u_off"] + C * g:L["u_off"] + C * (g + 1)] = uh
    h = rs.uniform(-1, 1, (n_src, C)).astype(np.float32) if has_h else None
    ep = rs.uniform(-0.1, 0.1, (G, 3, C)).astype(np.float32)
    # relu margin: resample V[j, g, c] until every out-edge of j has |V + W3 r| >= RELU_MARGIN (in fp64)
    reloc = min_image(torch.from_numpy(xs[src, :3]).double(), torch.from_numpy(xd[dst, :3]).double()).numpy()
    V = p_src[:, L["v_off"]:L["v_off"] + G * C].reshape(n_src, G, C)
    V[:] = rs.uniform(-1, 1, V.shape)
    for _ in range(200):
        pre = V[src].astype(np.float64) + np.einsum("ek,gkc->egc", reloc, ep.astype(np.float64))
        close = np.zeros((n_src, G, C), bool)
        np.logical_or.at(close, src, np.abs(pre) < RELU_MARGIN)
        if not close.any():
            break
        V[close] = rs.uniform(-1, 1, int(close.sum()))
    p_src[:, L["v_off"]:L["v_off"] + G * C] = V.reshape(n_src, G * C)
    g_agg = np.full((n_dst, L["ld_agg"]), 1e20, np.float32)   # columns the backward must not read: huge
    for g in range(G):
        base = g * L["a_gstride"]
        g_agg[:, base + L["a_off"]:base + L["a_off"] + C] = rs.uniform(-1, 1, (n_dst, C))
        g_agg[:, base + L["sc_off"]:base + L["sc_off"] + 2] = rs.uniform(-1, 1, (n_dst, 2))
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    return dict(ei=torch.from_numpy(np.stack([src, dst]).astype(np.int64)), ea=t(ea), xs=t(xs), xd=t(xd), p_src=t(p_src),
                p_dst=t(p_dst), h=t(h), ep=t(ep), g_agg=t(g_agg), n_src=n_src, n_dst=n_dst, deg=deg, kind=kind)


def run_sweep(be, prob, L, dev):
    """Forward + backward of one sweep problem on a backend (HipBackend on cuda, or the torch emulator on the cpu).
    Returns (csr info, einfo, agg, backward outputs), all on the CPU."""
    t = lambda a: None if a is None else a.to(dev)
    ei, n_src, n_dst, G = t(prob["ei"]), prob["n_src"], prob["n_dst"], L["G"]
    E = ei.size(1)
    csr = be.build_csr(ei, n_src, n_dst)
    rcsr = be.build_csr(ei.flip(0).contiguous(), n_dst, n_src)
    inv = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    if E:
        inv[csr.perm[:E].long()] = torch.arange(E, dtype=torch.int32, device=dev)
        r_slot = inv[rcsr.perm[:E].long()].contiguous()
    else:
        r_slot = torch.zeros(1, dtype=torch.int32, device=dev)
    einfo = torch.zeros(E + 3, 20, device=dev)
    be.edge_prepare([(csr, t(prob["ea"]), t(prob["xs"]), t(prob["xd"]), einfo)])
    agg = torch.zeros(n_dst, L["ld_agg"], device=dev)
    args = (t(prob["p_src"]), t(prob["p_dst"]), t(prob["h"]), t(prob["ep"]))
    be.aggregate(csr, einfo, *args, agg, *offsets(L))
    bwd = lambda: be.aggregate_backward(csr, rcsr, r_slot, einfo, *args, agg, t(prob["g_agg"]), *offsets(L))
    out = bwd()
    again = bwd()
    cpu = lambda a: None if a is None else a.detach().cpu()
    reproducible = all((a is None and b is None) or torch.equal(a, b) for a, b in zip(out, again))
    info = dict(rowptr=cpu(csr.rowptr)[:n_dst + 1].long(), col=cpu(csr.col)[:E].long(),
                perm=cpu(csr.perm)[:E].long() if E else torch.zeros(0, dtype=torch.long))
    return info, cpu(einfo), cpu(agg), tuple(cpu(a) for a in out), reproducible


def sweep_reference(prob, info, einfo, L, dtype=torch.float64):
    """The sweep restated in `dtype` and differentiated by autograd for the problem's g_agg.  Returns (forward
    {agg columns}, gradients {OUTPUTS}, magnitudes {OUTPUTS} (fp64 only; + "edge": per-edge alpha, ds and the g_sae term
    of S, for the checks' own tests), pre-activations V + W3 r [E, G, C]).
    The restatement: min-image relocation as the edge records hold it, s = u4 . x4 + u_h . h_j, segment softmax with
    +1e-16, relu(V_j + W3 r), the alpha-weighted sum, den = sum alpha, sae = sum alpha a."""
    G, n_src, n_dst = L["G"], prob["n_src"], prob["n_dst"]
    rowptr, col = info["rowptr"], info["col"]
    E = col.numel()
    dst = torch.repeat_interleave(torch.arange(n_dst), rowptr[1:] - rowptr[:-1])
    # the CSR is the one of the edge list, and the edge records hold the min-image relocation and the attribute
    assert torch.equal(rowptr, torch.cat([torch.zeros(1, dtype=torch.long),
                                          torch.bincount(prob["ei"][1], minlength=n_dst).cumsum(0)]))
    if E:
        assert torch.equal(col, prob["ei"][0][info["perm"]]) and torch.equal(dst, prob["ei"][1][info["perm"]])
    e32 = einfo[:E]
    want = min_image(prob["xs"][col, :3].double(), prob["xd"][dst, :3].double())
    assert _amax(e32[:, 16:19].double() - want) <= 1e-6, "edge records: min-image relocation"
    assert torch.equal(e32[:, 16:19], e32[:, 0:3]) and torch.equal(e32[:, 19], prob["ea"][info["perm"]])
    cast = lambda a: None if a is None else a.to(dtype)
    x4, reloc, a = cast(e32[:, :16]), cast(e32[:, 16:19]), cast(e32[:, 19])
    leaves = {"p_src": cast(prob["p_src"]).requires_grad_(True), "p_dst": cast(prob["p_dst"]).requires_grad_(True),
              "ep": cast(prob["ep"]).requires_grad_(True)}
    has_h = prob["h"] is not None
    if has_h:
        leaves["h"] = cast(prob["h"]).requires_grad_(True)
    g_agg = cast(prob["g_agg"])
    fwd, pres, terms, tot = {}, [], [], 0.0
    with torch.enable_grad():
        for g in range(G):
            base = g * L["a_gstride"]
            V = leaves["p_src"][col, L["v_off"] + g * C:L["v_off"] + (g + 1) * C]
            s = (leaves["p_dst"][dst, L["u4_off"] + g * 16:L["u4_off"] + (g + 1) * 16] * x4).sum(-1)
            if has_h:
                s = s + (leaves["p_dst"][dst, L["u_off"] + g * C:L["u_off"] + (g + 1) * C] * leaves["h"][col]).sum(-1)
            smax = torch.full((n_dst,), float("-inf"), dtype=dtype).scatter_reduce(0, dst, s.detach(), "amax")
            p = (s - smax[dst]).exp()
            den = torch.zeros(n_dst, dtype=dtype).index_add(0, dst, p)
            alpha = p / (den[dst] + 1e-16)
            pre = V + reloc @ leaves["ep"][g]
            r = torch.relu(pre)
            out = torch.zeros(n_dst, C, dtype=dtype).index_add(0, dst, alpha[:, None] * r)
            sa = torch.zeros(n_dst, dtype=dtype).index_add(0, dst, alpha)
            sae = torch.zeros(n_dst, dtype=dtype).index_add(0, dst, alpha * a)
            go, gd, gs = g_agg[:, base + L["a_off"]:base + L["a_off"] + C], g_agg[:, base + L["sc_off"]], g_agg[:, base + L["sc_off"] + 1]
            tot = tot + (out * go).sum() + (sa * gd).sum() + (sae * gs).sum()
            fwd[g] = (out.detach(), sa.detach(), sae.detach())
            pres.append(pre.detach())
            terms.append((s.detach(), alpha.detach(), r.detach(), go, gd, gs))
        names = list(leaves)
        grads = dict(zip(names, torch.autograd.grad(tot, [leaves[k] for k in names], allow_unused=True)))
    z = lambda k, like: torch.zeros_like(like) if grads.get(k) is None else grads[k]
    ref = {"g_p_dst": z("p_dst", leaves["p_dst"]), "g_p_src": z("p_src", leaves["p_src"]),
           "g_h_src": z("h", leaves["h"]) if has_h else None, "g_ep": z("ep", leaves["ep"])}
    pre_all = torch.stack(pres, 1) if pres else torch.zeros(E, G, C, dtype=dtype)
    if dtype != torch.float64:
        return fwd, ref, None, pre_all
    # ---- fp64 magnitudes, element by element ----
    mag = {k: (None if v is None else torch.zeros_like(v)) for k, v in ref.items()}
    mag["edge"] = {"alpha": torch.zeros(E, G, dtype=dtype), "ds": torch.zeros(E, G, dtype=dtype),
                   "S_sae": torch.zeros(n_dst, G, dtype=dtype), "dst": dst, "col": col, "x4": x4}
    mag["fwd"] = {}
    P, H = prob["p_dst"].double(), (prob["h"].double() if has_h else None)
    for g, (s, alpha, r, go, gd, gs) in enumerate(terms):
        out, sa, sae = fwd[g]
        kap = (P[dst, L["u4_off"] + g * 16:L["u4_off"] + (g + 1) * 16].abs() * x4.abs()).sum(-1)
        if has_h:
            uh = P[:, L["u_off"] + g * C:L["u_off"] + (g + 1) * C]
            kap = kap + (uh[dst].abs() * H[col].abs()).sum(-1)
        kappa = torch.zeros(n_dst, dtype=dtype).scatter_reduce(0, dst, kap, "amax")
        dal = (go[dst] * r).sum(-1) + gd[dst] + gs[dst] * a
        S = (go * out).sum(-1) + gd * sa + gs * sae
        dmag = (go[dst].abs() * r.abs()).sum(-1) + gd[dst].abs() + (gs[dst] * a).abs()
        Smag = (go.abs() * out.abs()).sum(-1) + (gd * sa).abs() + (gs * sae).abs()
        # ds = alpha (dalpha - S): the cancellation of the difference, and alpha's own relative error (KAPPA_W kappa)
        dsm = alpha * (dmag + Smag[dst]) + alpha * (dal - S[dst]).abs() * KAPPA_W * kappa[dst]
        mag["edge"]["alpha"][:, g], mag["edge"]["ds"][:, g], mag["edge"]["S_sae"][:, g] = alpha, alpha * (dal - S[dst]), gs * sae
        mag["g_p_dst"][:, L["u4_off"] + g * 16:L["u4_off"] + (g + 1) * 16] += \
            torch.zeros(n_dst, 16, dtype=dtype).index_add(0, dst, dsm[:, None] * x4.abs())
        if has_h:
            mag["g_p_dst"][:, L["u_off"] + g * C:L["u_off"] + (g + 1) * C] += \
                torch.zeros(n_dst, C, dtype=dtype).index_add(0, dst, dsm[:, None] * H[col].abs())
            mag["g_h_src"] += torch.zeros(n_src, C, dtype=dtype).index_add(0, col, dsm[:, None] * uh[dst].abs())
        vm = alpha * (1 + KAPPA_W * kappa[dst])
        # the forward's own columns: sum alpha |r| (1 + KAPPA_W kappa), with |r| = 1 for sum alpha and |a| for sum alpha a
        mag["fwd"][g] = (torch.zeros(n_dst, C, dtype=dtype).index_add(0, dst, vm[:, None] * r.abs()),
                         torch.zeros(n_dst, dtype=dtype).index_add(0, dst, vm),
                         torch.zeros(n_dst, dtype=dtype).index_add(0, dst, vm * a.abs()))
        mag["g_p_src"][:, L["v_off"] + g * C:L["v_off"] + (g + 1) * C] += \
            torch.zeros(n_src, C, dtype=dtype).index_add(0, col, vm[:, None] * go[dst].abs())
        mag["g_ep"][g] += (reloc.abs().t() @ (vm[:, None] * go[dst].abs()))
    return fwd, ref, mag, pre_all


def forward_excess(agg, fwd, mag, L, tol=SWEEP_TOL):
    """{column group: (worst ratio, index)} of the forward sweep's columns of `agg` -- the aggregate, sum alpha and
    sum alpha a of every gate -- against the fp64 forward `fwd` of sweep_reference, each element against
    sum alpha |r| (1 + KAPPA_W kappa) (mag["fwd"]; |r| = 1 for sum alpha, |a| for sum alpha a); <= 1 passes.  The factor
    is alpha's relative error: it reaches every alpha-weighted sum of different terms (the aggregate, sum alpha a).  In
    sum alpha = den / (den + 1e-16) it cancels, so that column is graded more loosely than it could be
    (cellcheck.cell_magnitudes takes the term without the factor)."""
    res = {}
    for g in range(L["G"]):
        base = g * L["a_gstride"]
        got = (agg[:, base + L["a_off"]:base + L["a_off"] + C], agg[:, base + L["sc_off"]], agg[:, base + L["sc_off"] + 1])
        for name, a, b, m in zip(("agg", "sum_alpha", "sum_alpha_a"), got, fwd[g], mag["fwd"][g]):
            r = bound_excess(a.detach(), b.detach(), m.detach(), tol)
            if r[0] >= res.get(name, (-1.0, None))[0]:
                res[name] = (r[0], None if r[1] is None else (g,) + tuple(int(v) for v in r[1]))
    return res


def owned_columns(L, has_h):
    """{output: column mask} of the columns a sweep writes."""
    G = L["G"]
    md = torch.zeros(L["ldp_dst"], dtype=torch.bool)
    md[L["u4_off"]:L["u4_off"] + 16 * G] = True
    if has_h:
        md[L["u_off"]:L["u_off"] + C * G] = True
    ms = torch.zeros(L["ldp_src"], dtype=torch.bool)
    ms[L["v_off"]:L["v_off"] + C * G] = True
    return {"g_p_dst": md, "g_p_src": ms}


def bound_excess(got, ref, mag, tol, floor_rel=1e-9):
    """max over elements of |got - ref| / (tol * mag + floor), floor = floor_rel * max(mag) (+1e-30); and its index."""
    d = (got.double() - ref.double()).abs()
    floor = floor_rel * float(mag.max()) + 1e-30 if mag.numel() else 1e-30
    r = d / (tol * mag.double() + floor)
    if r.numel() == 0:
        return 0.0, None
    k = int(torch.argmax(r))
    return float(r.reshape(-1)[k]), np.unravel_index(k, r.shape)


def sweep_excess(got, ref, mag, L, has_h, tol=SWEEP_TOL):
    """{output: (worst ratio, index)} of the four backward outputs against the fp64 reference (<= 1 passes).  The
    columns of g_p_dst / g_p_src a sweep does not own are compared exactly (to the reference's zeros)."""
    res = {}
    cols = owned_columns(L, has_h)
    for k, name in enumerate(OUTPUTS):
        a, b, m = got[k], ref[name], mag[name]
        if b is None:
            assert a is None, name
            continue
        if name == "g_ep" and a.dim() == 4:     # (partials, from ep_partial_out)
            a = a.sum(0)
        if name in cols:
            assert torch.equal(a[:, ~cols[name]], torch.zeros_like(a[:, ~cols[name]])), f"{name}: columns it does not own"
            a, b, m = a[:, cols[name]], b[:, cols[name]], m[:, cols[name]]
        res[name] = bound_excess(a, b, m, tol)
    return res


def check_relu_margin(pre):
    m = float(pre.abs().min()) if pre.numel() else 1.0
    assert m >= RELU_MARGIN * (1 - 1e-6), f"a pre-activation V + W3 r is {m:.2e} from 0: the reference would be ambiguous"


# --------------------------------------------------------------------------------------------------------------------
# Heads (models.py:427-452 regressor, 595-609 classifier): fp64 autograd of the recorded formulation
# --------------------------------------------------------------------------------------------------------------------
HEAD_TOL = 2e-5
# y = tanh in fp32 is off by <= 2 ulps of 1 = 2.4e-7 absolute, so 1 - y^2 by <= 4.8e-7 |y| absolute (all of it where
# tanh saturates): 0.024 |y| in units of HEAD_TOL
TANH_SAT = 4.8e-7 / HEAD_TOL
# ... and the fp32 pre-activation p carries ~4 eps kappa (kappa = sum |h| |w| + |b|): 1 - tanh(p)^2 moves by a relative
# 2 |y| of that, 0.024 kappa in units of HEAD_TOL
KAPPA_H = 8 * 2.0 ** -24 * 2 / HEAD_TOL / 2


def _tanh_mag(g, y, kappa):
    """Magnitude of g * (1 - y^2) as fp32 forms it: y = tanh(p) with p of magnitude kappa."""
    return g.abs() * ((1 - y * y) * (1 + KAPPA_H * kappa) + TANH_SAT * y.abs())


def regressor_heads_ref(hj, hg, xg, wj, bj, wg, bg, want, scaling=20.0, dtype=torch.float64):
    """fp64 (or `dtype`) autograd of models.py:427-452 for the incoming gradients `want` = (g_yj, g_yg, g_area), each
    a tensor or None.  h may be wider than the weights (padded channels, exactly zero): only the first columns are read.
    Returns (grads {hj, hg, wj, bj, wg, bg}, magnitudes of the same shapes)."""
    w = wj.size(1)
    cast = lambda t: t.detach().to(dtype).requires_grad_(True)
    L = {k: cast(v) for k, v in (("hj", hj), ("hg", hg), ("wj", wj), ("bj", bj), ("wg", wg), ("bg", bg))}
    with torch.enable_grad():
        pj = L["hj"][:, :w] @ L["wj"].t() + L["bj"]
        pg = L["hg"][:, :w] @ L["wg"].t() + L["bg"]
        yj = torch.tanh(pj)
        area = torch.tanh(pg[:, 0]) / scaling + xg[:, 3].to(dtype)
        yg = torch.stack([torch.tanh(pg[:, 0]), torch.relu(pg[:, 1])], 1)
        outs = [(o, g.to(dtype)) for o, g in zip((yj, yg, area), want) if g is not None]
        names = list(L)
        gr = torch.autograd.grad([o for o, _ in outs], [L[k] for k in names], [g for _, g in outs], allow_unused=True)
    ref = {k: (torch.zeros_like(L[k]) if g is None else g) for k, g in zip(names, gr)}
    z = lambda n: torch.zeros(n, dtype=torch.float64)
    g_yj, g_yg, g_ar = (None if g is None else g.double() for g in want)
    tj, tg = yj.detach().double(), torch.tanh(pg[:, 0].detach().double())
    kj = hj[:, :w].double().abs() @ wj.double().abs().t() + bj.double().abs()
    kg = hg[:, :w].double().abs() @ wg.double().abs().t() + bg.double().abs()
    mj = torch.zeros_like(tj) if g_yj is None else _tanh_mag(g_yj, tj, kj)
    gt = (z(hg.size(0)) if g_yg is None else g_yg[:, 0].abs()) + (z(hg.size(0)) if g_ar is None else g_ar.abs() / scaling)
    mg = torch.stack([_tanh_mag(gt, tg, kg[:, 0]),
                      z(hg.size(0)) if g_yg is None else g_yg[:, 1].abs() * (pg[:, 1].detach() > 0).double()], 1)
    Hj, Hg = hj.double().abs(), hg.double().abs()
    mag = {"hj": torch.zeros_like(Hj), "hg": torch.zeros_like(Hg)}
    mag["hj"][:, :w] = mj @ wj.double().abs()
    mag["hg"][:, :w] = mg @ wg.double().abs()
    mag["wj"], mag["bj"] = mj.t() @ Hj[:, :w], mj.sum(0)
    mag["wg"], mag["bg"] = mg.t() @ Hg[:, :w], mg.sum(0)
    return ref, mag


def classifier_heads_ref(h, ea, W, b, src, dst, want, dtype=torch.float64):
    """fp64 autograd of models.py:595-609 (pair = [h[src] | h[dst] | len], edge = tanh(lin1 pair), edge_event =
    lin2 pair) for `want` = (g_edge [E, 2], g_event [E]), each a tensor or None.  Returns (grads {h, W, b}, magnitudes)."""
    cast = lambda t: t.detach().to(dtype).requires_grad_(True)
    L = {"h": cast(h), "W": cast(W), "b": cast(b)}
    with torch.enable_grad():
        pair = torch.cat([L["h"][src], L["h"][dst], ea.to(dtype).view(-1, 1)], 1)
        y = pair @ L["W"].t() + L["b"]
        edge, event = torch.tanh(y[:, :2]), y[:, 2]
        outs = [(o, g.to(dtype)) for o, g in zip((edge, event), want) if g is not None]
        gr = torch.autograd.grad([o for o, _ in outs], [L[k] for k in L], [g for _, g in outs], allow_unused=True)
    ref = {k: (torch.zeros_like(L[k]) if g is None else g) for k, g in zip(L, gr)}
    E, n = src.numel(), h.size(0)
    t = edge.detach().double()
    m = torch.zeros(E, 3, dtype=torch.float64)
    if want[0] is not None:
        pa = torch.cat([h[src], h[dst], ea.view(-1, 1)], 1).double().abs()
        m[:, :2] = _tanh_mag(want[0].double(), t, pa @ W[:2].double().abs().t() + b[:2].double().abs())
    if want[1] is not None:
        m[:, 2] = want[1].double().abs()
    H, Wa = h.double().abs(), W.double().abs()
    mag = {"W": torch.cat([m.t() @ H[src], m.t() @ H[dst], (m * ea.double().abs().view(-1, 1)).sum(0)[:, None]], 1),
           "b": m.sum(0),
           "h": torch.zeros(n, C, dtype=torch.float64).index_add(0, src, m @ Wa[:, :C]).index_add(0, dst, m @ Wa[:, C:2 * C])}
    return ref, mag


def heads_excess(got, ref, mag, tol=HEAD_TOL):
    return {k: bound_excess(got[k], ref[k], mag[k], tol) for k in ref}


# --------------------------------------------------------------------------------------------------------------------
# Relu kinks of the gradient fuzz, proven from an fp64 record of every PeriodConv
# --------------------------------------------------------------------------------------------------------------------
GRAD_RTOL, GRAD_ATOL = 2e-4, 1e-6
# A relu mask may fall on the other side of 0 where the product's projection V = lin_value(x_j) is within its own rounding
# of 0.  That arithmetic (two-piece fp16 / split products, fp32 sums in another order) was measured at 5e-7 of
# sum_k |x_k| |W_ck| + |b_c|; TAU = 2e-6 is four times that: an fp64 pre-activation farther from 0 than TAU times its own
# magnitude cannot flip, and an edge that can is named in the proof.
TAU = 2e-6
MAX_KINK_ROWS = 2
MAX_EXCUSED = 4


@contextlib.contextmanager
def record_periodconvs(model, tag):
    """Records, for every PeriodConv of `model` (forward hooks and a tensor hook; the model is not changed):
    x_j (input of lin_value), pre = lin_value(x_j), lin_value's weight and bias, and the gradient at the relu output
    (input of lin_l2), per call.  Yields {f"{tag}/{module name}": record}."""
    rec, handles = {}, []
    for name, mod in model.named_modules():
        if not (hasattr(mod, "lin_value") and hasattr(mod, "lin_l2")):
            continue
        r = rec.setdefault(f"{tag}/{name}", {"x": [], "pre": [], "g": [], "W": mod.lin_value.weight, "b": mod.lin_value.bias})

        def on_value(m, inp, out, r=r):
            r["x"].append(inp[0].detach())
            r["pre"].append(out.detach())

        def on_l2(m, inp, r=r):
            t = inp[0]
            if t.requires_grad:
                k = len(r["g"])
                r["g"].append(None)
                t.register_hook(lambda g, k=k: r["g"].__setitem__(k, g.detach()))

        handles += [mod.lin_value.register_forward_hook(on_value), mod.lin_l2.register_forward_pre_hook(on_l2)]
    try:
        yield rec
    finally:
        for hd in handles:
            hd.remove()


def _record_of(name, records):
    for suffix in (".lin_value.weight", ".lin_value.bias"):
        if name.endswith(suffix):
            return records.get(name[:-len(suffix)]), suffix
    return None, None


def judge_tensor(name, got, ref, gmax, records):
    """One parameter gradient against its fp64 value.  Returns (ok, excuse): excuse = None (within the bar) or a list of
    (row c, [(edge, |pre|, flip bound of the row's worst column)]) -- a relu kink proven by the record, or ok = False.
    The bar: 2e-4 * max|ref| + 1e-6 * (largest gradient entry of the model).  Beyond it a tensor is excused only if it is a
    lin_value weight / bias with at most two bad rows c, each with edges e where |pre[e, c]| <= TAU (|x_j[e]| . |W_c| +
    |b_c|), and the row's deviation at most sum over those edges of |g_relu_out[e, c]| |[x_j | 1][e, k]| (1 + 1e-3) + bar."""
    got, ref = got.double(), ref.double()
    bar = GRAD_RTOL * _amax(ref) + GRAD_ATOL * gmax
    d = (got - ref).abs()
    if _amax(d) <= bar:
        return True, None
    r, suffix = _record_of(name, records)
    if r is None or not r["x"] or any(g is None for g in r["g"]):
        return False, None
    d = d.reshape(d.size(0), -1)
    bad = torch.nonzero(d.max(1).values > bar).reshape(-1).tolist()
    if len(bad) > MAX_KINK_ROWS:
        return False, None
    x = torch.cat([t.double() for t in r["x"]])
    pre = torch.cat([t.double() for t in r["pre"]])
    g = torch.cat([t.double() for t in r["g"]])
    W = r["W"].detach().double()
    bias = r["b"].detach().double() if r["b"] is not None else torch.zeros(W.size(0), dtype=torch.float64)
    xbar = torch.cat([x, torch.ones(x.size(0), 1, dtype=torch.float64)], 1)
    xbar = xbar[:, :-1] if suffix == ".lin_value.weight" else xbar[:, -1:]
    proof = []
    for c in bad:
        near = pre[:, c].abs() <= TAU * (x.abs() @ W[c].abs() + bias[c].abs())
        if not bool(near.any()):
            return False, None
        flip = (g[near, c].abs()[:, None] * xbar[near].abs()).sum(0) * (1 + 1e-3)
        if bool((d[c] > flip + bar).any()):
            return False, None
        k = int(torch.argmax(d[c]))
        proof.append((c, [(int(e), float(pre[e, c].abs()), float(flip[k])) for e in torch.nonzero(near).reshape(-1).tolist()]))
    return True, proof


def judge_gradients(got, ref, records):
    """All parameter gradients of a case.  Returns (failures [(name, err / max|ref|)], excused [(name, proof)]).  More than
    MAX_EXCUSED excused tensors fail the case (reported as a failure named '<too many kinks>')."""
    gmax = max(_amax(g) for g in ref.values())
    fails, excused = [], []
    for n, g in ref.items():
        ok, proof = judge_tensor(n, got[n], g, gmax, records)
        if not ok:
            fails.append((n, float((got[n].double() - g.double()).abs().max()) / max(_amax(g), 1e-300)))
        elif proof is not None:
            excused.append((n, proof))
    if len(excused) > MAX_EXCUSED:
        fails.append(("<too many kinks>", float(len(excused))))
    return fails, excused


# --------------------------------------------------------------------------------------------------------------------
# Gradient fuzz cases (tests/fuzz_training.py's draw)
# --------------------------------------------------------------------------------------------------------------------
def fuzz_params(rs):
    """The script's draw of one case's structure: (n_grains, lattice noise, weight seed, weight scale, voronoi seed)."""
    n_g = int(rs.choice([12, 40, 150, 400]))
    noise = None if rs.rand() < 0.5 else float(rs.uniform(0.05, 0.3))
    wseed, scale = int(rs.randint(1, 10 ** 6)), float(rs.choice([0.5, 1.0, 2.0]))
    return n_g, noise, wseed, scale, int(rs.randint(1, 10 ** 6))


def fuzz_data(rs, n_g, noise, vseed):
    """The structure and its random targets / masks / labels, drawn from `rs` in the script's order."""
    from graingraphnn_amd import synthetic
    x, ei, ea = synthetic.voronoi(n_g, seed=vseed, lattice_noise=noise)
    n_j, n_gr, E = x["joint"].shape[0], x["grain"].shape[0], ei[JJ].shape[1]
    y = {"joint": rs.uniform(-1, 1, (n_j, 2)).astype(np.float32), "grain": rs.uniform(-1, 1, (n_gr, 2)).astype(np.float32),
         "edge_event": rs.randint(-1, 2, size=E).astype(np.int64)}
    mask = {"joint": (rs.rand(n_j, 1) > 0.1).astype(np.float32), "grain": (rs.rand(n_gr, 1) > 0.1).astype(np.float32)}
    return x, ei, ea, y, mask


def model_grads(R, Cm, x, ei, ea, y, mask, dev, dtype=torch.float32):
    """Losses and every parameter gradient of both models (train.py's two losses), as the fuzz takes them."""
    from helpers import tt
    from graingraphnn_amd import training
    R.train(), Cm.train()
    R.zero_grad(), Cm.zero_grad()
    cast = lambda d: {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in tt(d, dev).items()}
    Y, M = cast(y), cast(mask)
    lr = training.regressor_loss(Y, R(cast(x), tt(ei, dev), cast(ea)), M)
    lc = training.classifier_loss(Y, Cm(cast(x), tt(ei, dev), cast(ea)), 1.0)
    lr.backward()
    lc.backward()
    out = {}
    for tag, m in (("R", R), ("C", Cm)):
        for n, p in m.named_parameters():
            out[f"{tag}/{n}"] = (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu()
    return float(lr.detach()), float(lc.detach()), out


def oracle_fp64_grads(wseed, scale, x, ei, ea, y, mask):
    """fp64 oracle gradients with the PeriodConv records of both models: (loss_r, loss_c, grads, records, models)."""
    from helpers import oracle_models
    oR, oC = oracle_models(wseed, scale)
    oR, oC = oR.double(), oC.double()
    with record_periodconvs(oR, "R") as rr, record_periodconvs(oC, "C") as rc:
        lr, lc, g = model_grads(oR, oC, x, ei, ea, y, mask, "cpu", torch.float64)
    return lr, lc, g, {**rr, **rc}, (oR, oC)


def format_excuse(name, proof):
    rows = "; ".join(f"row {c}: " + ", ".join(f"edge {e} |pre| {p:.2e} flip bound {f:.2e}" for e, p, f in edges[:3])
                     + (f" (+{len(edges) - 3} edges)" if len(edges) > 3 else "") for c, edges in proof)
    return f"excused relu kink {name}: {rows}"
