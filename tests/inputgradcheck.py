"""Checking code of the input gradients: the fp64 restatement of one sweep with the edge record's parts as
leaves, mapped back to the node rows and the edge attribute the record was made from, with per-element fp64 magnitudes
built the way gradcheck builds them; and the model-level cases (inputs as leaves of both models, both modes).

Nothing here reads the HIP path's output to set a bound: the sweep bound is gradcheck.SWEEP_TOL times the fp64 magnitude
of the element's own sum, the model bar is gradcheck.GRAD_RTOL / GRAD_ATOL, the bar of the parameter gradients.
"""
import numpy as np
import torch

import gradcheck as gc
from gradcheck import C, KAPPA_W, SWEEP_TOL

INPUT_OUTPUTS = ("g_x_src", "g_x_dst", "g_edge_attr")
GX_COLS = 16   # width of the node-gradient buffers the tests hand to the sweep: columns behind the owned ones stay zero


def run_sweep_inputs(be, prob, L, dev):
    """gradcheck.run_sweep with the input gradients requested: forward + backward of one sweep problem on the HIP backend.
    Returns (csr info, einfo, agg, the four existing outputs, the existing outputs of a call WITHOUT input gradients,
    {INPUT_OUTPUTS}, reproducible), all on the CPU."""
    t = lambda a: None if a is None else a.to(dev)
    ei, n_src, n_dst = t(prob["ei"]), prob["n_src"], prob["n_dst"]
    E, Fs = ei.size(1), prob["xs"].size(1)
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
    be.aggregate(csr, einfo, *args, agg, *gc.offsets(L))

    def bwd(with_inputs=True):
        gxs, gxd, gea = torch.zeros(n_src, GX_COLS, device=dev), torch.zeros(n_dst, GX_COLS, device=dev), torch.zeros(E, device=dev)
        kw = {"inputs": (Fs, gxs, gxd, gea, False, False)} if with_inputs else {}
        out = be.aggregate_backward(csr, rcsr, r_slot, einfo, *args, agg, t(prob["g_agg"]), *gc.offsets(L), **kw)
        return tuple(out) + (gxs, gxd, gea)

    out, again, plain = bwd(), bwd(), bwd(False)
    cpu = lambda a: None if a is None else a.detach().cpu()
    reproducible = all((a is None and b is None) or torch.equal(a, b) for a, b in zip(out, again))
    info = dict(rowptr=cpu(csr.rowptr)[:n_dst + 1].long(), col=cpu(csr.col)[:E].long(),
                perm=cpu(csr.perm)[:E].long() if E else torch.zeros(0, dtype=torch.long))
    return (info, cpu(einfo), cpu(agg), tuple(cpu(a) for a in out[:4]), tuple(cpu(a) for a in plain[:4]),
            dict(zip(INPUT_OUTPUTS, (cpu(a) for a in out[4:]))), reproducible)


def map_back(g_x4, g_r, g_a, info, dst, n_src, n_dst, Fs, sign=-1.0):
    """The record's gradient mapped through its column map: columns 0..2 (+ g_r) are the relocation x_src - x_dst (+ a
    piecewise constant shift), 3..Fs-1 the source's features, 13 (+ the direct term g_a) the edge attribute, through perm.
    `sign` = -1: the destination side; +1 for magnitudes (sums of absolute values)."""
    col, perm = info["col"], info["perm"]
    E = col.numel()
    g_reloc = g_x4[:, :3] + g_r
    gxs = torch.zeros(n_src, GX_COLS, dtype=g_x4.dtype)
    gxs[:, :Fs] = torch.zeros(n_src, Fs, dtype=g_x4.dtype).index_add(0, col, torch.cat([g_reloc, g_x4[:, 3:Fs]], 1))
    gxd = torch.zeros(n_dst, GX_COLS, dtype=g_x4.dtype)
    gxd[:, :3] = torch.zeros(n_dst, 3, dtype=g_x4.dtype).index_add(0, dst, sign * g_reloc)
    gea = torch.zeros(E, dtype=g_x4.dtype)
    gea[perm] = g_x4[:, 13] + g_a
    return {"g_x_src": gxs, "g_x_dst": gxd, "g_edge_attr": gea}


def input_reference(prob, info, einfo, L, dtype=torch.float64):
    """The sweep restated in `dtype` (gradcheck.sweep_reference's restatement) with the edge record's parts -- x4 [E, 16],
    reloc [E, 3], a [E] -- as leaves, differentiated for the problem's g_agg and mapped back by `map_back`.
    Returns (gradients {INPUT_OUTPUTS}, magnitudes {INPUT_OUTPUTS} + "edge" (fp64 only: per-edge g_reloc [E, 3], the direct
    attribute term [E], dst), pre-activations [E, G, C]).  Magnitudes, per element of the record and then mapped like the
    gradient itself with absolute values: dsm |u4| for g_x4, vm |g_out| |W3| for g_r, alpha |g_sae| for the direct term,
    with dsm and vm as gradcheck.sweep_reference forms them for g_p_dst and g_p_src."""
    G, n_src, n_dst = L["G"], prob["n_src"], prob["n_dst"]
    rowptr, col = info["rowptr"], info["col"]
    E, Fs = col.numel(), prob["xs"].size(1)
    dst = torch.repeat_interleave(torch.arange(n_dst), rowptr[1:] - rowptr[:-1])
    cast = lambda a: None if a is None else a.to(dtype)
    e32 = einfo[:E]
    x4, reloc, a = (cast(v).clone().requires_grad_(True) for v in (e32[:, :16], e32[:, 16:19], e32[:, 19]))
    p_src, p_dst, ep, h, g_agg = (cast(prob[k]) for k in ("p_src", "p_dst", "ep", "h", "g_agg"))
    has_h = h is not None
    zero = lambda *s: torch.zeros(*s, dtype=dtype)
    if E == 0:
        z = map_back(zero(0, 16), zero(0, 3), zero(0), info, dst, n_src, n_dst, Fs)
        return z, ({**{k: v.clone() for k, v in z.items()}, "edge": {"g_reloc": zero(0, 3), "direct": zero(0), "dst": dst}}
                   if dtype == torch.float64 else None), zero(0, G, C)
    terms, pres, tot = [], [], 0.0
    with torch.enable_grad():
        for g in range(G):
            base = g * L["a_gstride"]
            V = p_src[col, L["v_off"] + g * C:L["v_off"] + (g + 1) * C]
            u4 = p_dst[dst, L["u4_off"] + g * 16:L["u4_off"] + (g + 1) * 16]
            s = (u4 * x4).sum(-1)
            if has_h:
                s = s + (p_dst[dst, L["u_off"] + g * C:L["u_off"] + (g + 1) * C] * h[col]).sum(-1)
            smax = torch.full((n_dst,), float("-inf"), dtype=dtype).scatter_reduce(0, dst, s.detach(), "amax")
            p = (s - smax[dst]).exp()
            den = zero(n_dst).index_add(0, dst, p)
            alpha = p / (den[dst] + 1e-16)
            pre = V + reloc @ ep[g]
            r = torch.relu(pre)
            out = zero(n_dst, C).index_add(0, dst, alpha[:, None] * r)
            sa = zero(n_dst).index_add(0, dst, alpha)
            sae = zero(n_dst).index_add(0, dst, alpha * a)
            go, gd, gs = g_agg[:, base + L["a_off"]:base + L["a_off"] + C], g_agg[:, base + L["sc_off"]], g_agg[:, base + L["sc_off"] + 1]
            tot = tot + (out * go).sum() + (sa * gd).sum() + (sae * gs).sum()
            pres.append(pre.detach())
            terms.append((alpha.detach(), r.detach(), out.detach(), sa.detach(), sae.detach(), go, gd, gs, u4))
        g_x4, g_r, g_a = torch.autograd.grad(tot, [x4, reloc, a])
    ref = map_back(g_x4, g_r, g_a, info, dst, n_src, n_dst, Fs)
    pre_all = torch.stack(pres, 1)
    if dtype != torch.float64:
        return ref, None, pre_all
    m_x4, m_r, m_a = zero(E, 16), zero(E, 3), zero(E)
    X4, A_ = x4.detach(), a.detach()
    for g, (alpha, r, out, sa, sae, go, gd, gs, u4) in enumerate(terms):
        kap = (u4.abs() * X4.abs()).sum(-1)
        if has_h:
            kap = kap + (p_dst[dst, L["u_off"] + g * C:L["u_off"] + (g + 1) * C].abs() * h[col].abs()).sum(-1)
        kappa = zero(n_dst).scatter_reduce(0, dst, kap, "amax")
        dal = (go[dst] * r).sum(-1) + gd[dst] + gs[dst] * A_
        S = (go * out).sum(-1) + gd * sa + gs * sae
        dmag = (go[dst].abs() * r.abs()).sum(-1) + gd[dst].abs() + (gs[dst] * A_).abs()
        Smag = (go.abs() * out.abs()).sum(-1) + (gd * sa).abs() + (gs * sae).abs()
        dsm = alpha * (dmag + Smag[dst]) + alpha * (dal - S[dst]).abs() * KAPPA_W * kappa[dst]
        vm = alpha * (1 + KAPPA_W * kappa[dst])
        m_x4 += dsm[:, None] * u4.abs()
        m_r += (vm[:, None] * go[dst].abs()) @ ep[g].abs().t()
        m_a += alpha * gs[dst].abs()
    mag = map_back(m_x4, m_r, m_a, info, dst, n_src, n_dst, Fs, sign=1.0)
    mag["edge"] = {"g_reloc": (g_x4[:, :3] + g_r).detach(), "direct": g_a.detach(), "dst": dst}
    return ref, mag, pre_all


def input_excess(got, ref, mag, Fs, tol=SWEEP_TOL):
    """{output: (worst ratio, index)} of the three input gradients against the fp64 reference, per element (<= 1 passes).
    The columns a sweep does not own -- behind Fs of a source row, behind the coordinates of a destination row -- must be
    exactly zero."""
    res = {}
    for name, owned in (("g_x_src", Fs), ("g_x_dst", 3)):
        a = got[name]
        assert torch.equal(a[:, owned:], torch.zeros_like(a[:, owned:])), f"{name}: columns it does not own"
        res[name] = gc.bound_excess(a[:, :owned], ref[name][:, :owned], mag[name][:, :owned], tol)
    res["g_edge_attr"] = gc.bound_excess(got["g_edge_attr"], ref["g_edge_attr"], mag["g_edge_attr"], tol)
    return res


# --------------------------------------------------------------------------------------------------------------------
# Model level: x_dict and edge_attr as leaves of both models
# --------------------------------------------------------------------------------------------------------------------
def narrow_models(layer_size, seed, scale, device):
    """(product regressor, classifier), (oracle regressor, classifier) at a layer size below 96, same seeded weights."""
    from oracle import grainnn_oracle as oracle
    from graingraphnn_amd import synthetic
    from graingraphnn_amd.models import GrainNN_classifier, GrainNN_regressor
    from graingraphnn_amd.seeding import load_seeded
    out = []
    for R_cls, C_cls, dev in ((GrainNN_regressor, GrainNN_classifier, device), (oracle.GrainNN_regressor, oracle.GrainNN_classifier, "cpu")):
        hp = synthetic.default_hyper(dev)
        hp.layer_size = layer_size
        R = R_cls(hp)
        Cm = C_cls(hp, R)
        load_seeded(R, seed, scale).eval()
        load_seeded(Cm, seed + 1, scale).eval()
        out.append((R.to(dev), Cm.to(dev)))
    return out


def input_names(x, ea):
    return [f"x/{nt}" for nt in sorted(x)] + ["ea/" + "__".join(et) for et in sorted(ea)]


def model_input_grads(model, which, x, ei, ea, y, mask, dev, dtype=torch.float32, train=True, inputs_require_grad=True):
    """One loss of one model ('R': training.regressor_loss, 'C': training.classifier_loss) with x_dict and edge_attr as
    leaves: (loss, {input name: gradient}, {parameter name: gradient}), on the CPU.  The model's mode is left as set here."""
    from helpers import tt
    from graingraphnn_amd import training
    model.train(train)
    model.zero_grad()
    cast = lambda d: {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in tt(d, dev).items()}
    X, EA, Y, M = cast(x), cast(ea), cast(y), cast(mask)
    if inputs_require_grad:
        for d in (X, EA):
            for v in d.values():
                v.requires_grad_(True)
    pred = model(X, tt(ei, dev), EA)
    loss = training.regressor_loss(Y, pred, M) if which == "R" else training.classifier_loss(Y, pred, 1.0)
    loss.backward()
    gin = {}
    if inputs_require_grad:
        for nt in sorted(X):
            gin[f"x/{nt}"] = (torch.zeros_like(X[nt]) if X[nt].grad is None else X[nt].grad).detach().cpu()
        for et in sorted(EA):
            gin["ea/" + "__".join(et)] = (torch.zeros_like(EA[et]) if EA[et].grad is None else EA[et].grad).detach().cpu()
    gpar = {n: (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().clone() for n, p in model.named_parameters()}
    return float(loss.detach()), gin, gpar


def assert_no_relu_kink(records):
    """No fp64 pre-activation of any recorded PeriodConv lies within gradcheck.TAU of its own magnitude from zero: no relu
    mask of the fp32 arithmetic can fall on the other side, so a gradient is held to its bar without an excuse."""
    n = 0
    for name, r in records.items():
        W = r["W"].detach().double().abs()
        b = r["b"].detach().double().abs() if r["b"] is not None else torch.zeros(W.size(0), dtype=torch.float64)
        for x, pre in zip(r["x"], r["pre"]):
            near = pre.double().abs() <= gc.TAU * (x.double().abs() @ W.t() + b)
            assert not bool(near.any()), f"{name}: {int(near.sum())} pre-activations within TAU of zero (choose another seed)"
            n += pre.numel()
    assert n > 0, "no PeriodConv was recorded"


def tensor_bar(ref, gmax):
    """The bar of the parameter gradients (gradcheck.judge_tensor): GRAD_RTOL * max|ref| + GRAD_ATOL * (largest entry)."""
    return gc.GRAD_RTOL * float(ref.abs().max() if ref.numel() else 0.0) + gc.GRAD_ATOL * gmax
