"""The training backward against fp64, at its edges: the sweep backward (ggnn_period_gat_aggregate_backward) and its
shared-buffer contract, the heads' backward (`_RegressorHeads`, `_ClassifierHeads`), and the gradient fuzz with relu kinks
proven from an fp64 record instead of assumed.  The CPU tests at the end show that each check sees a one-term bug.

Bounds are per element (tests/gradcheck.py): |hip - ref64| <= tol * (fp64 magnitude of the element's own sum) + a tiny
floor, so a small row is held to its own size and not to the tensor's largest entry.
"""
import numpy as np
import pytest
import torch

import gradcheck as gc
from emulator import TorchEmulatorBackend
from helpers import EDGE_TYPES, load_graph, product_models, tt

GJ, JG, JJ = ("grain", "push", "joint"), ("joint", "pull", "grain"), ("joint", "connect", "joint")


def _layout(variant):
    enc, dec = gc.training_layouts()
    G, has_h, lay = (4, True, dec) if variant == "decoder" else (3, False, enc)
    return gc.sweep_layout(G, GJ, lay["grain"], lay["joint"]), has_h


def _sweep_case(variant, seed, empty=False):
    L, has_h = _layout(variant)
    kw = dict(n_src=7, n_dst=5, empty=True) if empty else {}
    return L, has_h, gc.sweep_problem(L, has_h, seed, **kw)


def _agg_of(fwd, L, n_dst):
    """A forward {gate: (aggregate, sum alpha, sum alpha a)} laid out as the sweep writes its agg rows."""
    agg = torch.zeros(n_dst, L["ld_agg"], dtype=fwd[0][0].dtype if fwd else torch.float32)
    for g, (out, sa, sae) in fwd.items():
        base = g * L["a_gstride"]
        agg[:, base + L["a_off"]:base + L["a_off"] + 96] = out
        agg[:, base + L["sc_off"]], agg[:, base + L["sc_off"] + 1] = sa, sae
    return agg


# ---------------------------------------------------------------------------------------------------------------------
# 1. The sweep backward against the fp64 restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("variant,seed,empty", [("decoder", 1, False), ("encoder", 2, False), ("decoder", 3, True),
                                                ("encoder", 4, True)])
def test_hip_sweep_backward_against_fp64(variant, seed, empty):
    """All four outputs of aggregate_backward (u_h / u4 columns of g_p_dst, value columns of g_p_src, g_h_src, g_ep)
    against fp64 autograd of the restated sweep, per element against the fp64 magnitude of its own sum; the training
    layout's offsets and pitches; degrees 0-7, hubs of 900 and 3000, a source hub of 500, E = 0; scores over +-36 with
    the maximum in the first or the last unit, all-equal rows; no relu tie.  Bit-reproducible."""
    from graingraphnn_amd.backend import default_backend
    L, has_h, prob = _sweep_case(variant, seed, empty)
    info, einfo, agg, out, reproducible = gc.run_sweep(default_backend(), prob, L, "cuda")
    assert reproducible
    fwd, ref, mag, pre = gc.sweep_reference(prob, info, einfo, L)
    gc.check_relu_margin(pre)
    res = gc.sweep_excess(out, ref, mag, L, has_h)
    _, ref32, _, _ = gc.sweep_reference(prob, info, einfo, L, torch.float32)
    res32 = gc.sweep_excess(tuple(ref32[k] for k in gc.OUTPUTS), ref, mag, L, has_h)
    for k, (r, idx) in res.items():
        print(f"{variant} E={info['col'].numel()} {k}: worst |hip - ref64| / bound {r:.3f} at {idx} "
              f"(fp32 restatement: {res32[k][0]:.3f})")
    for k, (r, idx) in res.items():
        assert r <= 1.0, (variant, k, r, idx)
    # the forward split sweep on the same problem: its aggregate, sum alpha and sum alpha a columns of every gate
    fres = gc.forward_excess(agg, fwd, mag, L)
    fwd32, _, _, _ = gc.sweep_reference(prob, info, einfo, L, torch.float32)
    fres32 = gc.forward_excess(_agg_of(fwd32, L, prob["n_dst"]), fwd, mag, L)
    for k, (r, idx) in fres.items():
        print(f"{variant} E={info['col'].numel()} forward {k}: worst |hip - ref64| / bound {r:.3f} at {idx} "
              f"(fp32 restatement: {fres32[k][0]:.3f})")
    for k, (r, idx) in fres.items():
        assert r <= 1.0, (variant, "forward", k, r, idx)


# ---------------------------------------------------------------------------------------------------------------------
# 2. The shared-buffer contract of the sweeps of a cell (training.py's backward)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sweep_backward_shared_buffers_as_training_chains_them():
    """The three sweeps of the decoder cell as _PackedCell.backward chains them -- shared gP buffers, the second sweep out
    of the junctions given g_h_into= the first one's, ep_partial_out rows -- equal the independent calls: each sweep's
    own columns bit for bit, every other column (a sentinel, not zero) untouched, g_h the sum of the two sweeps, the
    partial rows summing to g_ep and the rows beyond aggregate_bwd_partials(n_dst) untouched."""
    from graingraphnn_amd.backend import default_backend
    from graingraphnn_amd.engine import alloc_einfo, graph_for
    from graingraphnn_amd.training import train_topology
    be = default_backend()
    _, dec = gc.training_layouts()
    G, SENT = 4, -7.25
    x, ei, ea = load_graph("40")
    X, EI, EA = ({k: v.cuda() for k, v in tt(t).items()} for t in (x, ei, ea))
    n = {nt: X[nt].size(0) for nt in X}
    graph = graph_for(be, EI, n)
    topo = train_topology(be, graph)
    einfo = alloc_einfo(graph, "cuda", zero=False)
    be.edge_prepare([(graph.csr[et], EA[et].reshape(-1), X[et[0]], X[et[-1]], einfo[et]) for et in EDGE_TYPES])
    gen = torch.Generator(device="cuda").manual_seed(11)
    mk = lambda *s: torch.rand(*s, device="cuda", generator=gen) * 2 - 1
    P = {nt: mk(n[nt], dec[nt].ncols) for nt in n}
    H = {nt: mk(n[nt], 96) for nt in n}
    ep = {et: mk(G, 3, 96) * 0.3 for et in EDGE_TYPES}
    agg = {nt: torch.zeros(n[nt], G * dec[nt].Kg, device="cuda") for nt in n}
    be.aggregate_batch([(graph.csr[et], einfo[et], P[et[0]], P[et[-1]], H[et[0]], ep[et], agg[et[-1]], dec[et[0]].v_off[et],
                         dec[et[-1]].u_off.get(et, 0), dec[et[-1]].u4_off[et], dec[et[-1]].a_off[et], dec[et[-1]].Kg,
                         dec[et[-1]].sc_off[et], G, 0) for et in EDGE_TYPES])
    g_agg = {nt: mk(n[nt], G * dec[nt].Kg) for nt in n}
    n_part = [be.aggregate_bwd_partials(n[et[-1]]) for et in EDGE_TYPES]
    assert len(set(n_part)) > 1                       # (the case training.py:281 zero-fills for)

    def sweep(et, **kw):
        s, d = et[0], et[-1]
        return be.aggregate_backward(topo.graph.csr[et], topo.rcsr[et], topo.r_slot[et], einfo[et], P[s], P[d], H[s], ep[et],
                                     agg[d], g_agg[d], dec[s].v_off[et], dec[d].u_off.get(et, 0), dec[d].u4_off[et],
                                     dec[d].a_off[et], dec[d].Kg, dec[d].sc_off[et], G, **kw)
    alone = {et: sweep(et) for et in EDGE_TYPES}
    gP = {nt: torch.full_like(P[nt], SENT) for nt in n}
    part = torch.full((len(EDGE_TYPES), max(n_part) + 2, G, 3, 96), SENT, device="cuda")
    gh_src = {nt: None for nt in n}
    for k, et in enumerate(EDGE_TYPES):
        s, d = et[0], et[-1]
        _, _, g_h, g_ep = sweep(et, out_p_dst=gP[d], out_p_src=gP[s], ep_partial_out=part[k], g_h_into=gh_src[s])
        assert g_ep is None
        if g_h is not None:
            gh_src[s] = g_h
    owned = {nt: torch.zeros(dec[nt].ncols, dtype=torch.bool) for nt in n}
    for k, et in enumerate(EDGE_TYPES):
        s, d = et[0], et[-1]
        cd = list(range(dec[d].u4_off[et], dec[d].u4_off[et] + 16 * G)) + list(range(dec[d].u_off[et], dec[d].u_off[et] + 96 * G))
        cs = list(range(dec[s].v_off[et], dec[s].v_off[et] + 96 * G))
        assert not owned[d][cd].any() and not owned[s][cs].any()     # the sweeps' columns are disjoint
        owned[d][cd], owned[s][cs] = True, True
        assert torch.equal(gP[d][:, cd], alone[et][0][:, cd]), (et, "g_p_dst")
        assert torch.equal(gP[s][:, cs], alone[et][1][:, cs]), (et, "g_p_src")
        assert bool((part[k, n_part[k]:] == SENT).all()), (et, "partial rows beyond aggregate_bwd_partials(n_dst)")
        got = part[k, :n_part[k]].sum(0)
        assert torch.allclose(got, alone[et][3], rtol=1e-6, atol=1e-6 * float(alone[et][3].abs().max())), et
    for nt in n:
        assert bool((gP[nt][:, ~owned[nt].cuda()] == SENT).all()), (nt, "columns no sweep owns")
    # joints: the source of (joint, pull, grain) and (joint, connect, joint); grains: of (grain, push, joint) alone
    assert torch.equal(gh_src["joint"], alone[JG][2] + alone[JJ][2])
    assert torch.equal(gh_src["grain"], alone[GJ][2])


# ---------------------------------------------------------------------------------------------------------------------
# 3. Heads
# ---------------------------------------------------------------------------------------------------------------------
SUBSETS = [(a, b, c) for a in (True, False) for b in (True, False) for c in (True, False) if a or b or c]


def _regressor_operands(nj, ng, width, seed, dev):
    g = torch.Generator().manual_seed(seed)
    hj, hg = torch.randn(nj, 96, generator=g), torch.randn(ng, 96, generator=g)
    hj[::5] *= 20.0                                   # saturating tanh
    hg[1::6] *= 20.0
    hj[:, width:], hg[:, width:] = 0.0, 0.0            # padded channels: exactly zero
    wj, wg = torch.randn(2, width, generator=g) * 0.2, torch.randn(2, width, generator=g) * 0.2
    bj, bg = torch.randn(2, generator=g) * 0.1, torch.tensor([0.3, 0.0])
    hg[0] = 0.0                                       # relu pre-activation exactly 0 (zero row, zero bias): gradient 0
    xg = torch.randn(ng, 11, generator=g)
    return [t.to(dev) for t in (hj, hg, xg, wj, bj, wg, bg)]


@pytest.mark.gpu
@pytest.mark.parametrize("nj,ng", [(1, 1), (15, 17), (16, 16), (17, 15), (1000, 20001), (20001, 1000)])
@pytest.mark.parametrize("width", [96, 64])
def test_regressor_heads_backward_against_fp64(nj, ng, width):
    """_RegressorHeads (ggnn_heads_regressor_backward + the wgrad / sum_rows pieces) against fp64 autograd of
    models.py:427-452, for every subset of (g_yj, g_yg, g_area) present; saturating tanh, negative and exactly-zero relu
    pre-activations; layer_size 96 and 64 (the padded path)."""
    from graingraphnn_amd.backend import default_backend
    from graingraphnn_amd.training import _RegressorHeads
    be = default_backend()
    ops = _regressor_operands(nj, ng, width, nj * 7 + ng + width, "cuda")
    hj, hg, xg, wj, bj, wg, bg = [t.clone().requires_grad_(i not in (2,)) for i, t in enumerate(ops)]
    yj, yg, area = _RegressorHeads.apply(hj, hg, xg, wj, bj, wg, bg, be)
    assert float(yg.detach()[0, 1]) == 0.0
    gen = torch.Generator().manual_seed(5)
    gy = [torch.randn(nj, 2, generator=gen), torch.randn(ng, 2, generator=gen), torch.randn(ng, generator=gen)]
    worst = 0.0
    for sub in SUBSETS:
        want = [g if on else None for g, on in zip(gy, sub)]
        outs = [(o, g.cuda()) for o, g in zip((yj, yg, area), want) if g is not None]
        got = torch.autograd.grad([o for o, _ in outs], [hj, hg, wj, bj, wg, bg], [g for _, g in outs], retain_graph=True,
                                  allow_unused=True)
        got = {k: (torch.zeros_like(r) if v is None else v).cpu() for k, v, r in zip(("hj", "hg", "wj", "bj", "wg", "bg"), got,
                                                                                       (hj, hg, wj, bj, wg, bg))}
        ref, mag = gc.regressor_heads_ref(*[t.cpu() for t in ops], want)
        for k, (r, idx) in gc.heads_excess(got, ref, mag).items():
            worst = max(worst, r)
            assert r <= 1.0, (sub, k, r, idx)
    print(f"regressor heads nj={nj} ng={ng} width={width}: worst |hip - ref64| / bound {worst:.3f}")


def _jj_graph(case, seed):
    """Junction-junction edges: 'hub' -- a junction with no out-edge, one with no in-edge, a hub of degree ~200,
    duplicate edges; 'one' -- E_jj = 1."""
    rs = np.random.RandomState(seed)
    if case == "one":
        return 6, np.array([[4], [2]])
    n = 300
    src, dst = rs.randint(2, n, 700), rs.randint(2, n, 700)
    src[:100], dst[100:200] = 7, 7                    # hub junction 7: 100 out + 100 in
    src[200:240], dst[200:240] = 11, 1                # junction 1: in-edges only (no out)
    src[240:280], dst[240:280] = 0, 13                # junction 0: out-edges only (no in)
    src[280:290], dst[280:290] = 21, 22               # duplicate edges
    keep = src != dst
    return n, np.stack([src[keep], dst[keep]])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["hub", "one"])
def test_classifier_heads_backward_against_fp64(case):
    """_ClassifierHeads (segment sums over the forward / reverse CSR, wgrad, [n, 6] products) against fp64 autograd of
    the pair formulation models.py:595-609; empty segments, a hub, duplicates, E_jj = 1; g_edge or g_event absent."""
    from graingraphnn_amd.backend import default_backend
    from graingraphnn_amd.engine import graph_for
    from graingraphnn_amd.training import _ClassifierHeads, train_topology
    be = default_backend()
    n, e = _jj_graph(case, 3)
    E = e.shape[1]
    EI = {GJ: torch.tensor([[0], [0]]).cuda(), JG: torch.tensor([[0], [0]]).cuda(), JJ: torch.from_numpy(e).cuda()}
    graph = graph_for(be, EI, {"grain": 2, "joint": n})
    topo = train_topology(be, graph)
    g = torch.Generator().manual_seed(17)
    h = torch.randn(n, 96, generator=g)
    h[3::4] *= 8.0                                     # some saturating tanh
    ea = torch.rand(E, generator=g) * 0.1
    W, b = torch.randn(3, 193, generator=g) * 0.3, torch.randn(3, generator=g) * 0.1
    hc, Wc, bc = (t.cuda().requires_grad_(True) for t in (h, W, b))
    edge, event = _ClassifierHeads.apply(hc, ea.cuda(), Wc, bc, be, topo)
    ge, gv = torch.randn(E, 2, generator=g), torch.randn(E, generator=g)
    src, dst = torch.from_numpy(e[0]).long(), torch.from_numpy(e[1]).long()
    worst = 0.0
    for want in ((ge, gv), (ge, None), (None, gv)):
        outs = [(o, t.cuda()) for o, t in zip((edge, event), want) if t is not None]
        got = torch.autograd.grad([o for o, _ in outs], [hc, Wc, bc], [t for _, t in outs], retain_graph=True)
        got = dict(zip(("h", "W", "b"), (t.cpu() for t in got)))
        ref, mag = gc.classifier_heads_ref(h, ea, W, b, src, dst, want)
        for k, (r, idx) in gc.heads_excess(got, ref, mag).items():
            worst = max(worst, r)
            assert r <= 1.0, (case, [w is not None for w in want], k, r, idx)
    print(f"classifier heads {case} (E={E}): worst |hip - ref64| / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# 4. The gradient fuzz in the suite: relu kinks proven, not assumed
# ---------------------------------------------------------------------------------------------------------------------
# (n_grains, lattice noise, weight seed, weight scale, voronoi seed) + the seed of the targets / masks / labels
FUZZ_CASES = [(12, None, 4242, 1.0, 811, 1), (12, 0.2, 9191, 2.0, 812, 2), (40, 0.12, 30303, 1.0, 813, 3),
              (150, None, 5150, 0.5, 814, 4), (150, 0.25, 6160, 2.0, 815, 5), (400, None, 7170, 1.0, 816, 6)]


def _fuzz_case_33():
    """Case 33 of the 60-case run (`fuzz_training.py --n 60 --seed 0`): the draws of cases 0-32 are replayed."""
    rs = np.random.RandomState(0)
    for it in range(34):
        n_g, noise, wseed, scale, vseed = gc.fuzz_params(rs)
        data = gc.fuzz_data(rs, n_g, noise, vseed)
    assert (n_g, wseed, scale, vseed) == (40, 872441, 0.5, 365602) and abs(noise - 0.15596) < 1e-5
    return wseed, scale, data


@pytest.mark.gpu
def test_gradient_fuzz_with_relu_kinks_proven():
    """Parameter gradients of the HIP training path against the fp64 oracle on seeded random structures (12 to 400
    grains, weight scales 0.5 / 1 / 2, round 6's case 33): every tensor within 2e-4 * max|ref| + 1e-6 * (largest entry),
    or a lin_value weight / bias whose <= 2 off rows are each proven a relu flip by the fp64 record (gradcheck.judge_tensor)."""
    import time
    t0 = time.time()
    cases = []
    for n_g, noise, wseed, scale, vseed, dseed in FUZZ_CASES:
        cases.append((f"{n_g} grains x{scale}", wseed, scale, gc.fuzz_data(np.random.RandomState(dseed), n_g, noise, vseed)))
    w33, s33, d33 = _fuzz_case_33()
    cases.append(("case 33", w33, s33, d33))
    failures = []
    for what, wseed, scale, (x, ei, ea, y, mask) in cases:
        R, Cm = product_models(wseed, scale, "cuda")
        la, lca, ga = gc.model_grads(R, Cm, x, ei, ea, y, mask, "cuda")
        lb, lcb, gb, records, _ = gc.oracle_fp64_grads(wseed, scale, x, ei, ea, y, mask)
        assert abs(la - lb) <= 1e-5 * abs(lb) and abs(lca - lcb) <= 1e-5 * abs(lcb), (what, la, lb, lca, lcb)
        fails, excused = gc.judge_gradients(ga, gb, records)
        atol = gc.GRAD_ATOL * max(float(g.abs().max()) for g in gb.values())
        kinked = {k for k, _ in excused}
        worst = max(float((ga[k].double() - g).abs().max()) / float(g.abs().max()) for k, g in gb.items()
                    if float(g.abs().max()) > 100 * atol and k not in kinked)
        print(f"{what}: worst per-tensor error {worst:.2e} (tensors above 1e-4 of the largest entry, kinks aside), "
              f"{len(excused)} excused", flush=True)
        for name, proof in excused:
            print("   " + gc.format_excuse(name, proof))
        failures += [(what, f) for f in fails]
    print(f"fuzz wall time {time.time() - t0:.0f} s")
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# 5. The checks themselves, on the CPU: each sees a one-term bug
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["decoder", "encoder"])
def test_sweep_check_accepts_the_emulator_and_sees_one_edge_bugs(variant):
    L, has_h, prob = _sweep_case(variant, 1)
    info, einfo, agg, out, _ = gc.run_sweep(TorchEmulatorBackend(), prob, L, "cpu")
    fwd, ref, mag, pre = gc.sweep_reference(prob, info, einfo, L)
    gc.check_relu_margin(pre)
    worst = lambda got: max(r for r, _ in gc.sweep_excess(got, ref, mag, L, has_h).values())
    assert worst(out) <= 0.2                          # the fp32 emulator: well inside the bound
    # the forward columns: the emulator and the fp32 restatement inside the bound, one edge's term of a hub row is not
    fworst = lambda a: max(r for r, _ in gc.forward_excess(a, fwd, mag, L).values())
    fwd32, _, _, _ = gc.sweep_reference(prob, info, einfo, L, torch.float32)
    print(f"{variant} forward: emulator {fworst(agg):.3f}, fp32 restatement {fworst(_agg_of(fwd32, L, prob['n_dst'])):.3f}")
    assert fworst(agg) <= 0.5 and fworst(_agg_of(fwd32, L, prob["n_dst"])) <= 0.5
    e = int(prob["deg"][:5].sum()) + 450              # an edge in the middle of the 900-edge hub row (row 5)
    bad = agg.clone()
    bad[5, L["sc_off"]] -= float(mag["edge"]["alpha"][e, 0])     # its alpha missing from gate 0's sum alpha
    assert fworst(bad) > 1.0
    ed, G = mag["edge"], L["G"]
    # (a) one edge's fp64 contribution removed from the 900-edge hub row (the edge of median |ds|)
    hub, rp = 5, info["rowptr"]
    assert prob["deg"][hub] == 900
    sl = torch.arange(int(rp[hub]), int(rp[hub + 1]))
    e = int(sl[ed["ds"][sl, 0].abs().argsort()[len(sl) // 2]])
    gp = out[0].clone()
    gp[hub, L["u4_off"]:L["u4_off"] + 16] -= (ed["ds"][e, 0] * ed["x4"][e]).float()
    if has_h:
        gp[hub, L["u_off"]:L["u_off"] + 96] -= (ed["ds"][e, 0] * prob["h"][ed["col"][e]].double()).float()
    assert worst((gp,) + out[1:]) > 1.0
    # (b) S without its g_sae term: ds_e grows by alpha_e g_sae sae_i
    d = ed["alpha"] * ed["S_sae"][ed["dst"]]
    gp = out[0].clone()
    for g in range(G):
        gp[:, L["u4_off"] + 16 * g:L["u4_off"] + 16 * (g + 1)] += torch.zeros(prob["n_dst"], 16, dtype=torch.float64).index_add(
            0, ed["dst"], d[:, g, None] * ed["x4"]).float()
    assert worst((gp,) + out[1:]) > 1.0
    # (c) one source row of g_h_src dropped (decoder) / of the value gradient (encoder: no hidden rows)
    j = 100
    assert int((prob["ei"][0] == j).sum()) > 0
    if has_h:
        gh = out[2].clone()
        gh[j] = 0.0
        assert worst(out[:2] + (gh,) + out[3:]) > 1.0
    else:
        gs = out[1].clone()
        gs[j, L["v_off"]:L["v_off"] + 96 * G] = 0.0
        assert worst((out[0], gs) + out[2:]) > 1.0


def test_heads_checks_see_one_term():
    """The heads' checks against their own fp32 evaluation pass; one row of g_h_joint moved by a single term (g_pre W of
    one output) or one element of the classifier's g_W moved by its largest single term fails."""
    ops = _regressor_operands(1000, 2001, 96, 3, "cpu")
    gen = torch.Generator().manual_seed(5)
    want = [torch.randn(1000, 2, generator=gen), torch.randn(2001, 2, generator=gen), torch.randn(2001, generator=gen)]
    ref, mag = gc.regressor_heads_ref(*ops, want)
    got, _ = gc.regressor_heads_ref(*ops, want, dtype=torch.float32)
    assert max(r for r, _ in gc.heads_excess(got, ref, mag).values()) <= 0.5
    hj, wj, bj = ops[0].double(), ops[3].double(), ops[4].double()
    gpre = want[0].double() * (1 - torch.tanh(hj @ wj.t() + bj) ** 2)
    n = int(torch.argmax(gpre[:, 0].abs() * (torch.arange(1000) % 5 != 0)))    # (a row whose tanh is not saturated)
    bad = dict(got)
    bad["hj"] = got["hj"].clone()
    bad["hj"][n] += (gpre[n, 0] * wj[0]).float()
    assert gc.heads_excess(bad, ref, mag)["hj"][0] > 1.0
    n, e = _jj_graph("hub", 3)
    g = torch.Generator().manual_seed(17)
    h, ea = torch.randn(n, 96, generator=g), torch.rand(e.shape[1], generator=g) * 0.1
    W, b = torch.randn(3, 193, generator=g) * 0.3, torch.randn(3, generator=g) * 0.1
    src, dst = torch.from_numpy(e[0]).long(), torch.from_numpy(e[1]).long()
    want = (torch.randn(e.shape[1], 2, generator=g), torch.randn(e.shape[1], generator=g))
    ref, mag = gc.classifier_heads_ref(h, ea, W, b, src, dst, want)
    got, _ = gc.classifier_heads_ref(h, ea, W, b, src, dst, want, dtype=torch.float32)
    assert max(r for r, _ in gc.heads_excess(got, ref, mag).values()) <= 0.5
    gp = want[1].double()                              # lin2: g_pre = g_event
    terms = gp * h[src, 40].double()                   # the terms of g_W[2, 40]
    bad = dict(got)
    bad["W"] = got["W"].clone()
    bad["W"][2, 40] += float(terms[terms.abs().argmax()])
    assert gc.heads_excess(bad, ref, mag)["W"][0] > 1.0


@pytest.fixture(scope="module")
def kink_case():
    """A small structure: fp64 oracle gradients with the PeriodConv records, and the fp32 oracle's gradients."""
    from helpers import oracle_models
    rs = np.random.RandomState(21)
    x, ei, ea, y, mask = gc.fuzz_data(rs, 12, None, 4321)
    wseed, scale = 777, 1.0
    lb, lcb, gb, rec, models = gc.oracle_fp64_grads(wseed, scale, x, ei, ea, y, mask)
    oR, oC = oracle_models(wseed, scale)
    _, _, g32 = gc.model_grads(oR, oC, x, ei, ea, y, mask, "cpu")
    return dict(data=(x, ei, ea, y, mask), wseed=wseed, scale=scale, gb=gb, rec=rec, g32=g32, models=models)


def test_kink_rule_accepts_the_fp32_oracle_and_rejects_a_corrupted_row(kink_case):
    gb, rec = kink_case["gb"], kink_case["rec"]
    fails, excused = gc.judge_gradients(kink_case["g32"], gb, rec)
    assert not fails, fails
    for name, proof in excused:
        print(gc.format_excuse(name, proof))
    gmax = max(float(g.abs().max()) for g in gb.values())
    name = max((k for k in gb if k.endswith(".lin_value.weight")), key=lambda k: float(gb[k].abs().max()))
    r = rec[name[:-len(".lin_value.weight")]]
    x, pre = torch.cat(r["x"]).double(), torch.cat(r["pre"]).double()
    W, bias = r["W"].detach().double(), r["b"].detach().double()
    near = (pre.abs() <= 1e3 * gc.TAU * (x.abs() @ W.abs().t() + bias.abs())).any(0)
    c = int(torch.nonzero(~near)[0])                  # a row with no pre-activation anywhere near 0
    bad = gb[name].clone()
    bad[c] += 1e-3 * float(gb[name].abs().max())
    ok, _ = gc.judge_tensor(name, bad, gb[name], gmax, rec)
    assert not ok
    # the same deviation on a lin_l2 tensor, and a lin_l2 tensor that carries a lin_value's exact flip: never excused
    l2 = name.replace("lin_value", "lin_l2")
    bad = gb[l2].clone()
    bad[c] += 1e-3 * float(gb[l2].abs().max())
    assert not gc.judge_tensor(l2, bad, gb[l2], gmax, rec)[0]


def test_kink_rule_accepts_one_exact_flip_and_rejects_twice_that(kink_case):
    """A channel whose pre-activation on one edge is moved to 1e-12 by shifting b_c: the gradient with that edge's relu
    mask flipped (exactly one term) is excused, twice that term is not, and the same deviation on lin_l2 is not."""
    from helpers import oracle_models
    x, ei, ea, y, mask = kink_case["data"]
    base = "R/gclstm_decoder.cell_list.0.conv_i.convs.joint__connect__joint"
    r = kink_case["rec"][base]
    pre, g = torch.cat(r["pre"]).double(), torch.cat(r["g"]).double()
    xb = torch.cat([torch.cat(r["x"]).double(), torch.ones(pre.size(0), 1, dtype=torch.float64)], 1)
    term = g.abs()[:, :, None] * xb.abs()[:, None, :]          # [E, C, K + 1]: the flip term of every (edge, channel)
    e, c = np.unravel_index(int(torch.argmax(term.amax(2))), term.shape[:2])
    oR, oC = oracle_models(kink_case["wseed"], kink_case["scale"])
    oR, oC = oR.double(), oC.double()
    mod = dict(oR.named_modules())[base[2:]].lin_value
    with torch.no_grad():                              # (in fp64: the shift lands within 1e-16 of its target)
        mod.bias[c] -= float(pre[e, c]) - 1e-12
    with gc.record_periodconvs(oR, "R") as rr, gc.record_periodconvs(oC, "C") as rc:
        _, _, gb = gc.model_grads(oR, oC, x, ei, ea, y, mask, "cpu", torch.float64)
    rec = {**rr, **rc}
    r = rec[base]
    pre, g = torch.cat(r["pre"]).double(), torch.cat(r["g"]).double()
    assert 0 < float(pre[e, c]) < 1e-10
    xb = torch.cat([torch.cat(r["x"]).double(), torch.ones(pre.size(0), 1, dtype=torch.float64)], 1)
    flip = g[e, c] * xb[e]                             # the term edge e adds to row c (mask on) -- removed by a flip
    gmax = max(float(t.abs().max()) for t in gb.values())
    for suffix, t in ((".lin_value.weight", flip[:-1]), (".lin_value.bias", flip[-1:])):
        name = base + suffix
        bar = gc.GRAD_RTOL * float(gb[name].abs().max()) + gc.GRAD_ATOL * gmax
        assert float(t.abs().max()) > 2 * bar          # (the term is visible)
        one, two = gb[name].clone(), gb[name].clone()
        one[c] -= t.reshape(one[c].shape)
        two[c] -= 2 * t.reshape(one[c].shape)
        ok, proof = gc.judge_tensor(name, one, gb[name], gmax, rec)
        assert ok and proof is not None and proof[0][0] == c and e in [k for k, _, _ in proof[0][1]], (name, proof)
        print(gc.format_excuse(name, proof))
        assert not gc.judge_tensor(name, two, gb[name], gmax, rec)[0], name
    l2 = base + ".lin_l2.bias"
    bad = gb[l2].clone()
    bad[c] -= float(flip[-1])
    assert float(flip[-1].abs()) > 2 * (gc.GRAD_RTOL * float(gb[l2].abs().max()) + gc.GRAD_ATOL * gmax)
    assert not gc.judge_tensor(l2, bad, gb[l2], gmax, rec)[0]
