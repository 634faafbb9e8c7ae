"""Validation metrics on CPU tensors (graingraphnn_amd.metrics: the torch fallback writes the device accumulator's layout):
against the goldens of the unmodified reference (tests/golden/make_golden_metrics.py), against the fp64 restatement
(tests/metriccheck.py) on inputs the goldens do not hold, the edge cases, the top-level shim and the C ABI of
ggnn_metric_record.  No GPU: tests/test_metrics_gpu.py runs the kernel against the same checks.

Bounds.  Counts, plist, rlist, test_auc, metric_list: EQUAL (the classifier's inputs satisfy the separation condition, which
is asserted; the regressor's counts involve no transcendental).  Sums against the reference: 1e-5 relative -- the reference
sums float32 products pairwise, (log2 n + a few) 6e-8 ~ 2e-6 over non-negative terms, times five.  Sums against the fp64
restatement: 1e-10 relative -- n 2^-53 with n <= 1e5 is 1.1e-11, times ten."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import metriccheck as mc
from helpers import GOLDEN, ROOT
from graingraphnn_amd import _lib
from graingraphnn_amd.metrics import edge_error_metric, feature_metric

REF_RTOL = 1e-5
F64_RTOL = 1e-10


def load(name):
    return np.load(os.path.join(GOLDEN, f"metrics_{name}.npz"))


def replay_golden(d, model_type, capsys, prefix="", device="cpu"):
    """Records a golden's batches epoch by epoch into a feature_metric on `device`; asserts everything the file holds."""
    metric, ref = feature_metric(model_type, 0), mc.Restatement(model_type)
    rec = 0
    for e, batches in enumerate(mc.golden_batches(d, prefix)):
        ref.reset()
        for b in batches:
            if model_type == "classifier":
                assert mc.separated(b["edge_event_logit"]).all()
            y, p, m = ({k: v.to(device) for k, v in part.items()} for part in mc.dicts(model_type, b))
            metric.record(y, p, m, e)
            ref.record(y, p, m, e)
            if model_type == "regressor":
                got, want = metric.acc_dicts, d[prefix + "acc_dicts"][rec]
                assert all(v >= 0 for v in got.values())
                worst = mc.rel([got[k] for k in mc.ACC_KEYS], want)
                assert worst <= REF_RTOL, (e, rec, worst)
            rec += 1
        mc.assert_matches(metric, ref, F64_RTOL, f"{prefix}{model_type} epoch {e}")
        capsys.readouterr()
        metric.epoch_summary()
        lines = capsys.readouterr().out
        assert metric.plist == d[prefix + "plist"][e].tolist() and metric.rlist == d[prefix + "rlist"][e].tolist()
        if d[prefix + "auc_is_int"][e]:
            assert isinstance(metric.test_auc, int) and metric.test_auc == 0
        else:
            assert metric.test_auc.dtype == torch.float32
            assert np.float32(float(metric.test_auc)) == d[prefix + "test_auc"][e]
        assert metric.metric_list == d[prefix + "metric_list"][:e + 1].tolist()
        assert lines == str(d[prefix + "lines"][e]), (lines, str(d[prefix + "lines"][e]))
        if model_type == "regressor":
            want = d[prefix + "acc_dicts"][rec - 1]
            errs = [100 * np.sqrt(want[k] / want[4 + k]) for k in (2, 3, 0, 1)]
            assert mc.rel([metric.x_err, metric.y_err, metric.s_err, metric.v_err], errs) <= REF_RTOL
        assert ref.lists()[1:] == (metric.plist, metric.rlist)
    return metric


# ---- goldens ------------------------------------------------------------------------------------------------------------
def test_regressor_golden(capsys):
    metric = replay_golden(load("regressor"), "regressor", capsys)
    metric.summary()
    assert capsys.readouterr().out == f"model id: 0 PR AUC {float(metric.test_auc)}\n"


def test_classifier_golden(capsys):
    replay_golden(load("classifier"), "classifier", capsys)


@pytest.mark.parametrize("model_type", ["regressor", "classifier"])
def test_no_valid_threshold_golden(model_type, capsys):
    metric = replay_golden(load("novalid"), model_type, capsys, prefix=model_type + "__")
    assert set(metric.plist) == set(metric.rlist) == {-1.0} and metric.test_auc == 0 and isinstance(metric.test_auc, int)


def test_regressor_golden_holds_scores_on_the_thresholds():
    """The fixture was built with scores EXACTLY equal to float32 thresholds (not positive: `<`), in counted rows."""
    d = load("regressor")
    thr = np.asarray(mc.thresholds("regressor"), np.float32)
    hits = sum(int((np.isin(b["grain_area"], thr) & (b["mask_grain"][:, 0] > 0)).sum()) for e in mc.golden_batches(d) for b in e)
    assert hits >= 20


def test_edge_error_metric_golden():
    d, ev = load("edge_error"), np.load(os.path.join(GOLDEN, "golden_cfg1_events.npz"))
    jj, jg = ("joint", "connect", "joint"), ("joint", "pull", "grain")
    for c, want in zip(d["cases"], d["errors"]):
        before, after = ({et: torch.from_numpy(ev[f"{c}__{side}_ei_" + "__".join(et)]) for et in (jj, jg)} for side in ("in", "out"))
        got = edge_error_metric(before, after) + edge_error_metric(after, before)
        assert got == tuple(want.tolist()), (c, got, want)


# ---- the torch fallback against the fp64 restatement on random inputs ---------------------------------------------------
@pytest.mark.parametrize("seed,ng,nj,ne", [(1, 1, 2, 1), (2, 63, 65, 64), (3, 257, 255, 1000), (4, 20000, 40000, 100000)])
def test_fallback_matches_restatement(seed, ng, nj, ne):
    rs = np.random.RandomState(seed)
    for model_type, make in (("regressor", lambda: mc.regressor_batch(rs, ng, nj)), ("classifier", lambda: mc.classifier_batch(rs, ne))):
        metric, ref = feature_metric(model_type, 0), mc.Restatement(model_type)
        for epoch in (0, 1):
            for _ in range(2):
                b = make()
                if model_type == "classifier":
                    assert mc.separated(b["edge_event_logit"]).all()
                loss = torch.tensor(float(rs.uniform(0.5, 2.0)), dtype=torch.float32)
                args = mc.dicts(model_type, b)
                metric.record(*args, epoch, loss=loss)
                ref.record(*args, epoch, loss=loss)
        mc.assert_matches(metric, ref, F64_RTOL, model_type)
        assert mc.rel(metric.mean_loss(), ref.mean_loss()) <= F64_RTOL


def test_host_loop_cost_model_counts_what_the_restatement_counts():
    """tests/metriccheck.py's HostLoop (arm (a) of tools/eval_epoch_ab.py) obtains the reference's way what the restatement
    states: same counts, same sums to float32 accuracy."""
    rs = np.random.RandomState(12)
    for model_type, make in (("regressor", lambda: mc.regressor_batch(rs, 60, 90)), ("classifier", lambda: mc.classifier_batch(rs, 200))):
        loop, ref = mc.HostLoop(model_type), mc.Restatement(model_type)
        for _ in range(2):
            args = mc.dicts(model_type, make())
            loop.record(*args, 0)
            ref.record(*args, 0)
        assert mc.rel(loop.err, ref.err) <= REF_RTOL and mc.rel(loop.norm, ref.norm) <= REF_RTOL
        tp, fp, fn = loop.summary()
        assert (tp, fp, fn) == (ref.tp.tolist(), ref.fp.tolist(), ref.fn.tolist())


# ---- edge cases ---------------------------------------------------------------------------------------------------------
def test_empty_batch():
    rs = np.random.RandomState(5)
    for model_type, b in (("regressor", mc.regressor_batch(rs, 0, 0)), ("classifier", mc.classifier_batch(rs, 0))):
        metric = feature_metric(model_type, 0)
        metric.record(*mc.dicts(model_type, b), 0)
        err, norm, loss, tp, fp, fn, batches = mc.accumulator(metric)
        assert not err.any() and not norm.any() and not tp.any() and not fp.any() and not fn.any() and batches == 0


def test_all_rows_masked_and_all_labels_unlabelled():
    rs = np.random.RandomState(6)
    b = mc.regressor_batch(rs, 50, 100)
    b["mask_grain"][:], b["mask_joint"][:] = 0, 0
    metric = feature_metric("regressor", 0)
    metric.record(*mc.dicts("regressor", b), 0)
    err, norm, _, tp, fp, fn, _ = mc.accumulator(metric)
    assert not err.any() and not norm.any() and not tp.any() and not fp.any() and not fn.any()
    with pytest.raises(ZeroDivisionError):
        metric.epoch_summary()
    b = mc.classifier_batch(rs, 300, labels=(-100,))
    metric = feature_metric("classifier", 0)
    metric.record(*mc.dicts("classifier", b), 0)
    assert not mc.accumulator(metric)[3].any() and not mc.accumulator(metric)[4].any() and not mc.accumulator(metric)[5].any()
    metric.epoch_summary()
    assert set(metric.plist) == {-1.0} and metric.test_auc == 0


def test_norms_accumulate_only_in_epoch_zero_and_survive_the_summary(capsys):
    rs = np.random.RandomState(7)
    metric = feature_metric("regressor", 0)
    metric.record(*mc.dicts("regressor", mc.regressor_batch(rs, 40, 80)), 0)
    norm0 = mc.accumulator(metric)[1].copy()
    assert (norm0 > 0).all()
    metric.epoch_summary()
    err, norm, _, tp, fp, fn, _ = mc.accumulator(metric)
    assert not err.any() and not tp.any() and not fp.any() and not fn.any() and np.array_equal(norm, norm0)
    metric.record(*mc.dicts("regressor", mc.regressor_batch(rs, 40, 80)), 1)
    err, norm = mc.accumulator(metric)[:2]
    assert (err > 0).all() and np.array_equal(norm, norm0)


def test_summary_without_an_epoch_zero_record_raises_zero_division():
    rs = np.random.RandomState(8)
    metric = feature_metric("regressor", 0)
    metric.record(*mc.dicts("regressor", mc.regressor_batch(rs, 40, 80)), 3)
    with pytest.raises(ZeroDivisionError):
        metric.epoch_summary()
    with pytest.raises(ZeroDivisionError):
        feature_metric("regressor", 0).epoch_summary()


def test_masked_row_with_non_finite_prediction_leaves_the_sums_finite():
    rs = np.random.RandomState(9)
    b = mc.regressor_batch(rs, 40, 80)
    b["mask_grain"][:3], b["mask_joint"][:2] = 0, 0
    b["p_grain"][0], b["p_grain"][1, 0], b["p_grain"][2, 1] = np.inf, np.nan, -np.inf
    b["p_joint"][0, 1], b["p_joint"][1] = np.nan, np.inf
    metric, ref = feature_metric("regressor", 0), mc.Restatement("regressor")
    metric.record(*mc.dicts("regressor", b), 0)
    ref.record(*mc.dicts("regressor", b), 0)
    assert np.isfinite(mc.accumulator(metric)[0]).all() and np.isfinite(ref.err).all()
    mc.assert_matches(metric, ref, F64_RTOL, "non-finite masked rows")


def special_counts(device="cpu"):
    """TP per threshold for single labelled-1 logits z = 0, 40, -40, -104 (one metric each)."""
    out = {}
    for z in (0.0, 40.0, -40.0, -104.0):
        metric = feature_metric("classifier", 0)
        metric.record({"edge_event": torch.tensor([1], device=device)}, {"edge_event": torch.tensor([z], dtype=torch.float32, device=device)}, {}, 0)
        _, _, _, tp, fp, fn, _ = mc.accumulator(metric)
        assert not fp.any() and np.array_equal(tp + fn, np.ones_like(tp))
        out[z] = tp.tolist()
    return out


def check_special_scores(tp):
    """Thresholds 1.0, 0.9, ..., 0.0 (index i = 1 - i / 10).  z = 0: the score is exactly 0.5, not positive at 0.5 (index 5),
    positive at 0.4 (index 6).  z = 40: exactly 1.0, never > 1.0, positive below.  z = -104: exp(104) overflows float32, the
    score is exactly 0.0, never > 0.0, positive nowhere.  z = -40: the float32 sigmoid is 4.2e-18, NOT 0.0 -- the reference
    (torch.sigmoid in float32, `> 0.0`) counts it positive at the threshold 0.0 and nowhere else, and so must this."""
    assert tp[0.0] == [0] * 6 + [1] * 5
    assert tp[40.0] == [0] + [1] * 10
    assert tp[-104.0] == [0] * 11
    s = torch.sigmoid(torch.tensor([-40.0]))
    assert float(s) > 0 and tp[-40.0] == [int(bool(s > t)) for t in mc.thresholds("classifier")] == [0] * 10 + [1]


def test_special_scores():
    check_special_scores(special_counts())


def test_mean_loss_and_its_reset(capsys):
    rs = np.random.RandomState(10)
    metric = feature_metric("classifier", 0)
    assert np.isnan(metric.mean_loss())
    for v in (1.0, 2.0, 4.5):
        metric.record(*mc.dicts("classifier", mc.classifier_batch(rs, 50)), 0, loss=torch.tensor(v))
    assert metric.mean_loss() == 2.5
    metric.epoch_summary()
    assert metric.mean_loss() == 2.5          # (the epoch's value, kept by the summary)
    assert mc.accumulator(metric)[2] == 0.0 and mc.accumulator(metric)[6] == 0
    metric.record(*mc.dicts("classifier", mc.classifier_batch(rs, 50)), 1, loss=torch.tensor(8.0))
    assert metric.mean_loss() == 8.0


def test_loss_meter_on_cpu():
    from graingraphnn_amd.training import LossMeter
    meter = LossMeter()
    assert np.isnan(meter.mean())
    for v in (0.25, 0.5, 1.5):
        meter.add(torch.tensor(v, requires_grad=True))
    assert meter.mean() == 0.75 and meter.total.dtype == torch.float64
    meter.reset()
    meter.add(torch.tensor([2.0]))
    assert meter.mean() == 2.0


# ---- the shim -----------------------------------------------------------------------------------------------------------
def test_top_level_shim_gives_our_class():
    code = "import metrics, graingraphnn_amd.metrics as m; " \
           "assert metrics.feature_metric is m.feature_metric and metrics.edge_error_metric is m.edge_error_metric; print('ok')"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_binding_lists_it():
    src = open(os.path.join(ROOT, "include", "ggnn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(ggnn_[a-z_0-9]+)\s*\(", src))) == sorted(_lib.EXPORTED_SYMBOLS)
    assert "ggnn_metric_record" in _lib.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "ggnn_metric_record")
    for name, value in (("MAX_TERMS", 4), ("MAX_THR", 16), ("BLOCKS", 64), ("F64_SLOTS", 9), ("I64_SLOTS", 49)):
        assert int(re.search(rf"#define GGNN_METRIC_{name} (\d+)", src).group(1)) == getattr(_lib, f"GGNN_METRIC_{name}") == value
    assert _lib.GGNN_METRIC_WS_WORDS == 64 * (8 + 48) + 1
    assert _lib.load().ggnn_version() == 26


def test_metric_args_size_matches_the_header():
    # pred, target, mask | n_rows, ld, ld_mask | col | score, label, label_mask | n, ld_label_mask | thr | loss, acc, workspace | 4 ints
    assert ctypes.sizeof(_lib.MetricArgs) == 3 * 4 * 8 + 3 * 4 * 8 + 4 * 4 + 3 * 8 + 2 * 8 + 16 * 4 + 3 * 8 + 4 * 4
    assert _lib.MetricArgs.thr.offset == 248 and _lib.MetricArgs.n_terms.offset == 336


def test_metric_record_validates_on_the_host():
    """EINVAL (-1) before anything is launched: the buffers are HOST memory, nothing may touch them."""
    lib = _lib.load()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p).value

    def args(**kw):
        a = _lib.MetricArgs()
        a.acc, a.workspace = p, p
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert lib.ggnn_metric_record(None, None) == -1
    a = args()
    a.acc = None
    assert lib.ggnn_metric_record(ctypes.byref(a), None) == -1            # a NULL accumulator
    a = args()
    a.workspace = None
    assert lib.ggnn_metric_record(ctypes.byref(a), None) == -1
    assert lib.ggnn_metric_record(ctypes.byref(args(n_thr=17)), None) == -1   # more than 16 thresholds
    assert lib.ggnn_metric_record(ctypes.byref(args(n_terms=5)), None) == -1  # more than four terms
    assert lib.ggnn_metric_record(ctypes.byref(args(n=-1)), None) == -1       # a negative count
    a = args(n_terms=1)
    a.n_rows[0] = -1
    assert lib.ggnn_metric_record(ctypes.byref(a), None) == -1
    a = args(n_terms=1)
    a.n_rows[0], a.ld[0], a.ld_mask[0] = 5, 2, 1                               # a non-empty term without operands
    assert lib.ggnn_metric_record(ctypes.byref(a), None) == -1
    assert lib.ggnn_metric_record(ctypes.byref(args(n=5, n_thr=3)), None) == -1   # elements without score / label
    assert lib.ggnn_metric_record(ctypes.byref(args(mode=2)), None) == -1
    assert not any(buf)
