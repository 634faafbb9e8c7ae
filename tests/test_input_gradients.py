"""Input gradients: loss.backward() through both models to x_dict and edge_attr.

  * sweep level: the three new outputs of ggnn_period_gat_aggregate_backward_inputs -- source rows, destination rows, edge
    attribute -- against the fp64 restatement with the edge record's parts as leaves, per element against the fp64
    magnitude of the element's own sum (tests/inputgradcheck.py), at gradcheck.SWEEP_TOL; bit-reproducible; the existing
    outputs bit-equal to a call without input gradients; columns that are not owned exactly zero;
  * model level: x_dict / edge_attr as leaves of both models against the fp64 oracle, per tensor at the bar of the
    parameter gradients, in .train() and in .eval(), at layer_size 96 and 64 -- on seeds for which the fp64 record proves
    that no relu can flip (asserted), so nothing is excused; parameter gradients bit-equal to a call without input gradients;
  * a two-step unrolled loss (training.unrolled_steps) against the same function on the fp64 oracle;
  * on the CPU: the new check accepts a float32 restatement and sees three one-term bugs; wants_autograd's routing.
"""
import functools

import numpy as np
import pytest
import torch

import gradcheck as gc
import inputgradcheck as igc
from emulator import TorchEmulatorBackend
from helpers import assert_close, oracle_models, product_models, tt

GJ = ("grain", "push", "joint")

# (grains, lattice noise, weight scale, voronoi seed, data seed) and, per differentiated model, the seed of the pair of
# models (helpers.oracle_models / product_models): chosen on the CPU so that no fp64 pre-activation of a PeriodConv of that
# model is within gradcheck.TAU of its own magnitude from zero (igc.assert_no_relu_kink, asserted again by every test that
# uses the case; about one seed in eight passes at 40 grains)
CASES = {"g12": (12, None, 1.0, 77, 5), "g40n": (40, 0.2, 1.0, 78, 6)}
WSEED = {("g12", "R"): 4101, ("g12", "C"): 4102, ("g40n", "R"): 4211, ("g40n", "C"): 4210}
NARROW = ("g12", 64, 33, 2.0)    # (case, layer_size, weight seed, weight scale) of the layer_size < 96 case (classifier)
DZ = 1.0 / 12


@functools.lru_cache(maxsize=None)
def _data(case):
    n_g, noise, _, vseed, dseed = CASES[case]
    return gc.fuzz_data(np.random.RandomState(dseed), n_g, noise, vseed)


def _models(case, which, layer, dev):
    """(product (R, C) on `dev` or None, oracle (R, C) in fp64) of the case that differentiates model `which`."""
    if layer == 96:
        wseed, scale = WSEED[case, which], CASES[case][2]
        return (None if dev is None else product_models(wseed, scale, dev)), tuple(m.double() for m in oracle_models(wseed, scale))
    prod, orc = igc.narrow_models(layer, NARROW[2], NARROW[3], dev or "cpu")
    return (None if dev is None else prod), tuple(m.double() for m in orc)


@functools.lru_cache(maxsize=None)
def _oracle_ref(case, which, layer=96):
    """fp64 oracle: (loss, input gradients, parameter gradients) of one case, computed once; no relu within TAU of zero."""
    _, (oR, oC) = _models(case, which, layer, None)
    m = oR if which == "R" else oC
    with gc.record_periodconvs(m, which) as rec:
        out = igc.model_input_grads(m, which, *_data(case), "cpu", torch.float64)
    igc.assert_no_relu_kink(rec)
    return out


def _judge_inputs(got, ref, what):
    gmax = max(gc._amax(g) for g in ref.values())
    assert gmax > 0
    worst = 0.0
    for n, g in ref.items():
        assert got[n].shape == g.shape, (n, got[n].shape, g.shape)
        err, bar = gc._amax(got[n].double() - g), igc.tensor_bar(g, gmax)
        print(f"{what} {n}: max|ref| {gc._amax(g):.3e}  |hip - ref64| {err:.3e}  bar {bar:.3e}  ratio {err / bar:.3f}")
        worst = max(worst, err / bar)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# 1. Sweep level, against fp64
# ---------------------------------------------------------------------------------------------------------------------
def _sweep_case(variant, seed, Fs, empty=False):
    enc, dec = gc.training_layouts()
    G, has_h, lay = (4, True, dec) if variant == "decoder" else (3, False, enc)
    L = gc.sweep_layout(G, GJ, lay["grain"], lay["joint"])
    kw = dict(n_src=7, n_dst=5, empty=True) if empty else {}
    return L, has_h, gc.sweep_problem(L, has_h, seed, Fs=Fs, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,seed,Fs,empty", [("decoder", 1, 11, False), ("encoder", 2, 8, False), ("decoder", 3, 11, True)])
def test_hip_sweep_input_gradients_against_fp64(variant, seed, Fs, empty):
    """g_x_src, g_x_dst and g_edge_attr of one sweep against fp64 autograd with x4, reloc and a as leaves, per element
    against dsm |u4| / vm |g_out| |W3| / alpha |g_sae| mapped like the gradient; degrees 0-7, hubs of 900 and 3000, the
    source hub, duplicate edges, E = 0; no relu tie.  Two calls bit-equal, the four existing outputs bit-equal to the entry
    point without input gradients, columns that are not owned exactly zero."""
    from graingraphnn_amd.backend import default_backend
    L, has_h, prob = _sweep_case(variant, seed, Fs, empty)
    info, einfo, agg, out, plain, got, reproducible = igc.run_sweep_inputs(default_backend(), prob, L, "cuda")
    assert reproducible
    for a, b, name in zip(out, plain, gc.OUTPUTS):
        assert (a is None and b is None) or torch.equal(a, b), f"{name} changed with the input gradients requested"
    ref, mag, pre = igc.input_reference(prob, info, einfo, L)
    gc.check_relu_margin(pre)
    ref32, _, _ = igc.input_reference(prob, info, einfo, L, torch.float32)
    res, res32 = igc.input_excess(got, ref, mag, Fs), igc.input_excess(ref32, ref, mag, Fs)
    for k, (r, idx) in res.items():
        print(f"{variant} f_src={Fs} E={info['col'].numel()} {k}: worst |hip - ref64| / bound {r:.3f} at {idx} "
              f"(fp32 restatement: {res32[k][0]:.3f})")
    for k, (r, idx) in res.items():
        assert r <= 1.0, (variant, k, r, idx)
    if not empty:
        assert all(gc._amax(got[k]) > 0 for k in igc.INPUT_OUTPUTS)


# ---------------------------------------------------------------------------------------------------------------------
# 2. Model level, against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case,which,train,layer", [(c, w, t, 96) for c in CASES for w in "RC" for t in (True, False)]
                         + [(NARROW[0], "C", True, NARROW[1])])
def test_model_input_gradients_against_fp64_oracle(case, which, train, layer):
    """.grad of every tensor of x_dict and edge_attr after loss.backward() through one model, in .train() and in .eval(),
    against the fp64 oracle with the same leaves: per tensor within GRAD_RTOL * max|ref| + GRAD_ATOL * (largest
    input-gradient entry), no relu excuse (the seeds keep every fp64 pre-activation farther than TAU from zero).  The
    parameter gradients of the same call are bit-equal to those of a call whose inputs do not require grad."""
    loss64, gin64, _ = _oracle_ref(case, which, layer)
    prod, _ = _models(case, which, layer, "cuda")
    m = prod[0] if which == "R" else prod[1]
    loss, gin, gpar = igc.model_input_grads(m, which, *_data(case), "cuda", train=train)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    worst = _judge_inputs(gin, gin64, f"{case} {which} {'train' if train else 'eval'} layer {layer}")
    _, _, gplain = igc.model_input_grads(m, which, *_data(case), "cuda", train=True, inputs_require_grad=False)
    differ = [n for n in gplain if not torch.equal(gpar[n], gplain[n])]
    assert not differ, f"parameter gradients moved with the input gradients requested: {differ[:5]}"
    assert any(gc._amax(g) > 0 for g in gplain.values())
    assert worst <= 1.0, worst


@pytest.mark.gpu
def test_grain_area_reaches_the_grain_areas():
    """grain_area = tanh(.) / scaling + x_grain[:, 3]: a loss on it alone adds its gradient to column 3 of x_dict['grain']
    (the regressor loss does not read grain_area) -- against the fp64 oracle, same bar."""
    case = "g12"
    x, ei, ea, y, mask = _data(case)
    prod, (oR, _) = _models(case, "R", 96, "cuda")
    w = torch.from_numpy(np.random.RandomState(3).uniform(0.5, 1.5, x["grain"].shape[0]))
    res = {}
    for name, m, dev, dt in (("hip", prod[0], "cuda", torch.float32), ("ref", oR, "cpu", torch.float64)):
        X = {k: v.to(dt).requires_grad_(True) for k, v in tt(x, dev).items()}
        EA = {k: v.to(dt) for k, v in tt(ea, dev).items()}
        with gc.record_periodconvs(m, "R") as rec:
            (m.train()(X, tt(ei, dev), EA)["grain_area"] * w.to(dev, dt)).sum().backward()
        if name == "ref":
            igc.assert_no_relu_kink(rec)
        res[name] = {f"x/{k}": v.grad.detach().cpu() for k, v in X.items()}
    assert _judge_inputs(res["hip"], res["ref"], "grain_area") <= 1.0
    assert gc._amax(res["ref"]["x/grain"][:, 3] - w) < 0.5 * float(w.min())    # (the direct term dominates the column)


# ---------------------------------------------------------------------------------------------------------------------
# 3. Unrolled: two differentiable steps
# ---------------------------------------------------------------------------------------------------------------------
def _unrolled(m, dev, dt, case="g12"):
    from graingraphnn_amd import training
    x, ei, ea, y, mask = _data(case)
    cast = lambda d: {k: (v.to(dt) if v.is_floating_point() else v) for k, v in tt(d, dev).items()}
    X, Y, M = cast(x), cast(y), cast(mask)
    X["joint"].requires_grad_(True)
    m.train()
    m.zero_grad()
    preds, states = training.unrolled_steps(m, X, tt(ei, dev), 2, DZ)
    loss = sum(training.regressor_loss(Y, p, M) for p in preds)
    loss.backward()
    gpar = {n: (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu() for n, p in m.named_parameters()}
    return float(loss.detach()), gpar, X["joint"].grad.detach().cpu(), {k: v.detach().cpu() for k, v in states[-1].items()}


@functools.lru_cache(maxsize=None)
def _unrolled_ref():
    _, (oR, _) = _models("g12", "R", 96, None)
    with gc.record_periodconvs(oR, "R") as rec:
        out = _unrolled(oR, "cpu", torch.float64)
    igc.assert_no_relu_kink(rec)
    return out


@pytest.mark.gpu
def test_unrolled_two_steps_against_fp64_oracle():
    """A loss over two consecutive regressor steps (training.unrolled_steps) differentiates end to end: the gradient of
    every regressor parameter and of (G, R) = x0['joint'][:, 3:5] against the same function on the fp64 oracle, at the bar
    of the parameter gradients; the final states agree within the forward tolerance."""
    loss64, gpar64, gx64, state64 = _unrolled_ref()
    prod, _ = _models("g12", "R", 96, "cuda")
    loss, gpar, gx, state = _unrolled(prod[0], "cuda", torch.float32)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    for nt in state64:
        assert_close(state[nt], state64[nt], f"unrolled state {nt}")
    gmax = max(gc._amax(g) for g in gpar64.values())
    bad = []
    for n, g in gpar64.items():
        err, bar = gc._amax(gpar[n].double() - g), igc.tensor_bar(g, gmax)
        if err > bar:
            bad.append((n, err, bar))
    print(f"unrolled: {len(gpar64)} parameter tensors, largest gradient entry {gmax:.3e}, over the bar: {bad}")
    assert not bad, bad
    ref = gx64[:, 3:5]
    err, bar = gc._amax(gx[:, 3:5].double() - ref), igc.tensor_bar(ref, gc._amax(ref))
    print(f"unrolled d loss / d (G, R): max|ref| {gc._amax(ref):.3e}  |hip - ref64| {err:.3e}  bar {bar:.3e}")
    assert gc._amax(ref) > 0 and err <= bar, (err, bar)


# ---------------------------------------------------------------------------------------------------------------------
# 4. CPU: the checks see bugs; routing; the unrolled step is the reference's update
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,Fs", [("decoder", 11), ("encoder", 8)])
def test_input_check_accepts_fp32_and_sees_one_term_bugs(variant, Fs):
    L, has_h, prob = _sweep_case(variant, 1, Fs)
    info, einfo, _, _, _ = gc.run_sweep(TorchEmulatorBackend(), prob, L, "cpu")
    ref, mag, pre = igc.input_reference(prob, info, einfo, L)
    gc.check_relu_margin(pre)
    got, _, _ = igc.input_reference(prob, info, einfo, L, torch.float32)
    worst = lambda g: max(r for r, _ in igc.input_excess(g, ref, mag, Fs).values())
    print(f"{variant}: fp32 restatement {worst(got):.3f}")
    assert worst(got) <= 1.0
    ed, col = mag["edge"], info["col"]
    # (a) one edge's relocation gradient sent to the wrong source row
    size = ed["g_reloc"].abs().max(1).values * (col != 3)          # (not an edge of the source hub)
    e = int(size.argmax())
    j, wrong = int(col[e]), (int(col[e]) + 1) % (prob["n_src"] - 20)
    assert wrong != 3 and int((prob["ei"][0] == wrong).sum()) > 0
    bad = {k: v.clone() for k, v in got.items()}
    bad["g_x_src"][j, :3] -= ed["g_reloc"][e].float()
    bad["g_x_src"][wrong, :3] += ed["g_reloc"][e].float()
    assert worst(bad) > 1.0
    # (b) the destination-side sign flipped
    bad = {k: v.clone() for k, v in got.items()}
    bad["g_x_dst"] = -bad["g_x_dst"]
    assert worst(bad) > 1.0
    # (c) the direct alpha g_sae term dropped from the attribute gradient
    bad = {k: v.clone() for k, v in got.items()}
    bad["g_edge_attr"][info["perm"]] -= ed["direct"].float()
    assert worst(bad) > 1.0


def test_input_gradient_entry_point_validates_without_launching():
    """The extension struct has the header's size; a missing or malformed one is GGNN_EINVAL (-1) before any launch."""
    import ctypes
    from graingraphnn_amd import _lib
    assert ctypes.sizeof(_lib.AggregateBwdInputs) == 5 * 8 + 2 * 8 + 4 * 4
    lib = _lib.load()
    a, x = _lib.AggregateBwdArgs(), _lib.AggregateBwdInputs()
    assert lib.ggnn_period_gat_aggregate_backward_inputs(None, None, None) == -1
    assert lib.ggnn_period_gat_aggregate_backward_inputs(ctypes.byref(a), None, None) == -1
    assert lib.ggnn_period_gat_aggregate_backward_inputs(ctypes.byref(a), ctypes.byref(x), None) == -1
    assert lib.ggnn_version() == _lib.GGNN_ABI_VERSION == 26


class _Params(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("leaf", [None, "x", "ea"])
def test_wants_autograd_routing(train, leaf):
    """Recording + an input that requires grad: the differentiable path in either mode.  No such input: .train() takes it,
    .eval() takes the fused path.  Under no_grad: always the fused path."""
    from graingraphnn_amd import training
    m = _Params().train(train)
    x = {"grain": torch.zeros(2, 11), "joint": torch.zeros(3, 8, requires_grad=leaf == "x")}
    ea = {GJ: torch.zeros(4, 1, requires_grad=leaf == "ea")}
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert training.wants_autograd(m, x, ea) is (train or leaf is not None)
        assert training.wants_autograd(m, x) is (train or leaf == "x")
        with torch.no_grad():
            assert training.wants_autograd(m, x, ea) is False


def test_unrolled_steps_is_the_reference_update():
    """training.unrolled_steps on the oracle regressor walks the states of the reference's loop (forward, update in place,
    z advanced and held at its clamp, edge lengths by the min-image) and carries gradients to the inputs of step 0."""
    from graingraphnn_amd import training
    x, ei, ea, _, _ = _data("g12")
    _, (oR, _) = _models("g12", "R", 96, None)
    X, EI = {k: v.double() for k, v in tt(x).items()}, tt(ei)
    X["grain"][:, 2] = X["joint"][:, 2] = 1.0 - 2.5 * DZ          # (the second step ends at the clamp)
    with torch.no_grad():
        S = {k: v.clone() for k, v in X.items()}
        for _ in range(2):
            EA = training.edge_lengths(S, EI)
            for et in EA:   # test.py:562-575
                rel = S[et[0]][EI[et][0], :2] - S[et[-1]][EI[et][1], :2]
                rel = -1 * (rel > 0.5) + 1 * (rel < -0.5) + rel
                assert torch.equal(EA[et], torch.sqrt(rel[:, 0] ** 2 + rel[:, 1] ** 2).view(-1, 1))
            oR.update(S, oR(S, EI, EA), {})
            S["grain"][:, 2] += DZ
            S["joint"][:, 2] += DZ
            if S["grain"][0, 2] > 1.0 - DZ:
                S["grain"][:, 2] = 1.0 - DZ
                S["joint"][:, 2] = 1.0 - DZ
    X["joint"].requires_grad_(True)
    preds, states = training.unrolled_steps(oR, X, EI, 2, DZ)
    assert len(preds) == len(states) == 2
    for nt in S:
        assert float((states[-1][nt] - S[nt]).abs().max()) <= 1e-12, nt
    assert float(states[-1]["grain"][0, 2]) == 1.0 - DZ
    assert torch.equal(states[-1]["grain"][:, :2], X["grain"][:, :2])          # centres held
    states[-1]["joint"][:, :2].sum().backward()
    assert X["joint"].grad is not None and float(X["joint"].grad[:, 3:5].abs().max()) > 0
