"""ggnn_metric_record on the GPU: the kernel behind graingraphnn_amd.metrics.feature_metric.record against the torch fallback
and the fp64 restatement (tests/metriccheck.py), bit-determinism across streams, hipGraph capture without a host stall, one
validation epoch of both models end to end, and training.LossMeter around GraphedTrainStep.

Bounds as in tests/test_metrics.py: counts EQUAL (classifier inputs satisfy the separation condition, asserted); fp64 sums
within 1e-10 relative of the restatement (n 2^-53, n <= 1e5, times ten); against the reference's float32 sums 1e-5."""
import numpy as np
import pytest
import torch

import metriccheck as mc
from helpers import load_graph, product_models, tt
from graingraphnn_amd import _lib, synthetic, training
from graingraphnn_amd.metrics import feature_metric
from test_metrics import F64_RTOL, REF_RTOL, check_special_scores, load, replay_golden, special_counts

pytestmark = pytest.mark.gpu
DEV = "cuda"
RAGGED = _lib.GGNN_METRIC_BLOCKS * 256 * 2 + 37   # every thread loops, the last round is ragged


def on_device(model_type, b):
    return tuple({k: v.to(DEV) for k, v in part.items()} for part in mc.dicts(model_type, b))


@pytest.mark.parametrize("model_type", ["regressor", "classifier"])
def test_kernel_on_the_goldens(model_type, capsys):
    replay_golden(load(model_type), model_type, capsys, device=DEV)


@pytest.mark.parametrize("model_type", ["regressor", "classifier"])
def test_kernel_on_the_no_valid_threshold_golden(model_type, capsys):
    replay_golden(load("novalid"), model_type, capsys, prefix=model_type + "__", device=DEV)


# (grain rows, joint rows, edges): wave and workgroup edges, one term empty, and the ragged many-rounds size
SHAPES = [(1, 1, 1), (63, 64, 63), (64, 65, 64), (65, 63, 65), (255, 257, 255), (257, 255, 257), (130, 0, 0), (0, 77, 300),
          (RAGGED, 2 * RAGGED + 1, RAGGED)]


@pytest.mark.parametrize("ng,nj,ne", SHAPES)
def test_kernel_matches_fallback_and_restatement(ng, nj, ne):
    rs = np.random.RandomState(ng + 3 * nj + 7 * ne)
    for model_type, make in (("regressor", lambda: mc.regressor_batch(rs, ng, nj)), ("classifier", lambda: mc.classifier_batch(rs, ne))):
        gpu, cpu, ref = feature_metric(model_type, 0), feature_metric(model_type, 0), mc.Restatement(model_type)
        for epoch in (0, 1):
            b = make()
            if model_type == "classifier":
                assert mc.separated(b["edge_event_logit"]).all()
            loss = torch.tensor(float(rs.uniform(0.5, 2.0)), dtype=torch.float32)
            gpu.record(*on_device(model_type, b), epoch, loss=loss.to(DEV))
            cpu.record(*mc.dicts(model_type, b), epoch, loss=loss)
            ref.record(*mc.dicts(model_type, b), epoch, loss=loss)
        assert gpu.acc.is_cuda and not cpu.acc.is_cuda
        mc.assert_matches(gpu, ref, F64_RTOL, f"kernel {model_type} {ng}/{nj}/{ne}")
        assert torch.equal(gpu.i64.cpu(), cpu.i64)
        assert mc.rel(gpu.f64.cpu().numpy(), cpu.f64.numpy()) <= 2 * F64_RTOL
        assert mc.rel(gpu.mean_loss(), ref.mean_loss()) <= F64_RTOL


def test_masked_row_with_non_finite_prediction_adds_exactly_zero():
    rs = np.random.RandomState(9)
    b = mc.regressor_batch(rs, 40, 80)
    clean = {k: v.copy() for k, v in b.items()}
    b["mask_grain"][:3], b["mask_joint"][:2] = 0, 0
    clean["mask_grain"][:3], clean["mask_joint"][:2] = 0, 0
    b["p_grain"][0], b["p_grain"][1, 0], b["p_grain"][2, 1] = np.inf, np.nan, -np.inf
    b["p_joint"][0, 1], b["p_joint"][1] = np.nan, np.inf
    got, want = feature_metric("regressor", 0), feature_metric("regressor", 0)
    got.record(*on_device("regressor", b), 0)
    want.record(*on_device("regressor", clean), 0)
    assert bool(torch.isfinite(got.f64).all()) and torch.equal(got.acc, want.acc)


def test_special_scores_on_the_device():
    check_special_scores(special_counts(DEV))


def test_fp64_slots_have_the_same_bits_on_every_run_and_stream():
    """The same nine records (the regressor golden's, all as epoch 0 so that the norms add too) three times: twice on the
    default stream, once on a side stream -- bit-equal accumulators."""
    batches = [on_device("regressor", b) + (torch.tensor(0.5 + k, device=DEV),)
               for k, b in enumerate(b for e in mc.golden_batches(load("regressor")) for b in e)]
    assert len(batches) == 9

    def run():
        metric = feature_metric("regressor", 0)
        for y, p, m, loss in batches:
            metric.record(y, p, m, 0, loss=loss)
        return metric
    a, b = run(), run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = run()
    side.synchronize()
    torch.cuda.synchronize()
    assert bool((a.f64[:8] > 0).all()) and int(a.i64[48]) == 9
    assert torch.equal(a.acc, b.acc) and torch.equal(a.acc, c.acc)


@pytest.mark.parametrize("model_type", ["regressor", "classifier"])
def test_record_is_capturable_and_never_synchronises(model_type):
    """record(..., loss=...) on static input buffers, captured once and replayed three times with new values copied in, adds
    what three eager records add, bit for bit -- and neither the eager records nor the copies and replays synchronise
    (torch's sync debug mode turns a synchronisation into an error); only epoch_summary() may."""
    rs = np.random.RandomState(21)
    make = (lambda: mc.regressor_batch(rs, 118, 236)) if model_type == "regressor" else (lambda: mc.classifier_batch(rs, 708))
    batches = [on_device(model_type, make()) + (torch.tensor(1.5 * (k + 1), device=DEV),) for k in range(3)]
    static = tuple({k: v.clone() for k, v in part.items()} for part in batches[0][:3]) + (batches[0][3].clone(),)
    graphed, eager = feature_metric(model_type, 0), feature_metric(model_type, 0)
    graphed.record(*static[:3], 0, loss=static[3])      # (warm-up: the accumulator exists before the capture)
    torch.cuda.synchronize()
    graphed.acc.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.record(*static[:3], 0, loss=static[3])
    torch.cuda.synchronize()
    assert not bool(graphed.acc.any())                  # (the capture only records)
    torch.cuda.set_sync_debug_mode("error")
    try:
        for y, p, m, loss in batches:
            for dst, src in zip(static[:3], (y, p, m)):
                for k in src:
                    dst[k].copy_(src[k])
            static[3].copy_(loss)
            graph.replay()
            eager.record(y, p, m, 0, loss=loss)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(graphed.acc, eager.acc) and int(eager.i64[48]) == 3
    ref = mc.Restatement(model_type)
    for y, p, m, loss in batches:
        ref.record(y, p, m, 0, loss=loss)
    mc.assert_matches(graphed, ref, F64_RTOL, f"captured {model_type}")


def test_validation_epoch_end_to_end_at_the_40um_graph(capsys):
    """Three validation batches of the 40 um fixture through both models (seeded weights, eval mode, no_grad), the losses
    and record(..., loss=loss); one epoch_summary().  The restatement gets the SAME predictions: only the metric is under
    test.  (The classifier's logits are the model's: those within the separation band are moved out of it first.)"""
    x, ei, ea = load_graph("40")
    R, Cm = product_models(10020, 1.0, DEV)
    EI = tt(ei, DEV)
    n_g, n_j, E = x["grain"].shape[0], x["joint"].shape[0], ei[synthetic.EDGE_TYPES[2]].shape[1]
    reg, cls = feature_metric("regressor", 0), feature_metric("classifier", 0)
    ref_r, ref_c = mc.Restatement("regressor"), mc.Restatement("classifier")
    with torch.no_grad():
        for k in range(3):
            rs = np.random.RandomState(300 + k)
            X, EA = tt(synthetic.perturbed_copy(x, 1e-3, 2000 + k), DEV), tt(ea, DEV)
            y = tt({"joint": rs.uniform(-0.1, 0.1, (n_j, 2)).astype(np.float32), "grain": rs.uniform(-0.1, 0.1, (n_g, 2)).astype(np.float32),
                    "grain_event": (rs.uniform(size=n_g) < 0.3).astype(np.int64), "edge_event": rs.randint(-1, 2, size=E).astype(np.int64)}, DEV)
            mask = tt({"joint": (rs.uniform(size=(n_j, 1)) > 0.1).astype(np.float32), "grain": (rs.uniform(size=(n_g, 1)) > 0.1).astype(np.float32)}, DEV)
            pred = R(X, EI, EA)
            loss = training.regressor_loss(y, pred, mask)
            reg.record(y, pred, mask, 0, loss=loss)
            ref_r.record(y, pred, mask, 0, loss=loss)
            pred = dict(Cm(X, EI, EA))
            pred["edge_event"] = torch.from_numpy(mc.separate(pred["edge_event"].cpu().numpy())).to(DEV)
            assert mc.separated(pred["edge_event"].cpu().numpy()).all()
            loss = training.classifier_loss(y, pred, 1.0)
            cls.record(y, pred, mask, 0, loss=loss)
            ref_c.record(y, pred, mask, 0, loss=loss)
    for metric, ref in ((reg, ref_r), (cls, ref_c)):
        mc.assert_matches(metric, ref, REF_RTOL, metric.model_type)
        metric.epoch_summary()
        assert mc.rel(metric.mean_loss(), ref.mean_loss()) <= REF_RTOL and np.isfinite(metric.mean_loss())
        area, ps, rs_ = ref.lists()
        assert (metric.plist, metric.rlist) == (ps, rs_) and float(metric.test_auc) == float(area)
    assert mc.rel([reg.x_err, reg.y_err, reg.s_err, reg.v_err], ref_r.errors()) <= REF_RTOL
    assert "Validation AUC" in capsys.readouterr().out


def test_loss_meter_over_graphed_train_steps():
    """training.LossMeter around ten GraphedTrainStep calls: no read-back per step; the mean equals the mean of the ten
    read-back losses within 1e-6 relative (ten float32 values summed in float64 either way)."""
    x, ei, ea = load_graph("40")
    A, _ = product_models(4, 1.0, DEV)
    X, EI, EA = tt(x, DEV), tt(ei, DEV), tt(ea, DEV)
    rs = np.random.RandomState(9)
    Y = {nt: torch.from_numpy(rs.uniform(-1, 1, (x[nt].shape[0], 2)).astype(np.float32)).to(DEV) for nt in x}
    mask = {nt: torch.ones(x[nt].shape[0], 1, device=DEV) for nt in x}
    opt = training.FusedAdam(A.parameters(), lr=1e-3)
    step = training.GraphedTrainStep(A, opt, lambda pred, y: training.regressor_loss(y, pred, mask), X, EI, EA, Y, warmup=2)
    meter, read = training.LossMeter(), []
    for _ in range(10):
        loss = step(X, EA, Y)
        meter.add(loss)
        read.append(float(loss.detach()))
    want = float(np.mean(np.asarray(read, np.float64)))
    assert len(set(read)) > 1 and abs(meter.mean() - want) <= 1e-6 * abs(want), (meter.mean(), want)
