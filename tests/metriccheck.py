"""float64 restatement (numpy) of the reference's validation metrics -- metrics.py:23-72 feature_metric.record, :74-109
epoch_summary, :124-217 grain_class_acc / class_acc -- for inputs the goldens of tests/golden/make_golden_metrics.py do not
cover, and the helpers the metric tests share.

    sums     err[k] = sum_r m (y - p)^2, norm[k] = sum_r m y^2 (epoch 0 only) over the float32 inputs taken to float64,
             k = grain0, grain1, joint0, joint1; a row with m == 0 adds exactly 0 (the project's choice where the reference's
             0 * inf is NaN).  np.sum's pairwise fp64 sum of n <= 1e5 non-negative terms: relative error <= n 2^-53.
    counts   regressor: rows with mask > 0, score = grain_area, positive = score < t;  classifier: labels > -1, score =
             sigmoid(logit), positive = score > t.  TP = (label 1, positive), FP = (label 0, positive), FN = (label 1, not
             positive).  The reference compares in float32 against the threshold rounded to float32; so does this (the regressor's
             scores are data, the classifier's sigmoid is float64 here and rounded to float32, which the SEPARATION condition
             makes immaterial: no score within 1e-5 of a threshold).
    summary  the reference's arithmetic on 0-dim int64 tensors (float32 quotients and area), from the counts.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_metrics as mgm  # noqa: E402  (the separation condition and the batch builders, shared with the goldens)

ACC_KEYS = mgm.ACC_KEYS
TERMS = (("grain", 0), ("grain", 1), ("joint", 0), ("joint", 1))
MAX_THR = 16
SEPARATION = mgm.SEPARATION
separated, separated_logits, regressor_batch, classifier_batch, dicts = \
    mgm.separated, mgm.separated_logits, mgm.regressor_batch, mgm.classifier_batch, mgm.dicts


def separate(logits):
    """The logits (float32 array) with every one that violates the separation condition moved by steps of 1e-3 until it
    holds: for logits a test cannot draw itself (a model's outputs); the metric under test and its restatement get the same."""
    z = np.array(logits, np.float32, copy=True)
    for _ in range(100):
        bad = ~separated(z)
        if not bad.any():
            return z
        z[bad] += np.float32(1e-3)
    raise AssertionError("could not separate the logits from the thresholds")


def thresholds(model_type):
    return mgm.REGRESSOR_THRESHOLDS if model_type == "regressor" else mgm.CLASSIFIER_THRESHOLDS


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


class Restatement:
    """The accumulator's layout on the host: err[4], norm[4] (float64), tp / fp / fn [n_thr] (Python ints), loss, batches."""

    def __init__(self, model_type):
        self.model_type = model_type
        self.thr32 = np.asarray(thresholds(model_type), np.float64).astype(np.float32)
        self.norm = np.zeros(4)
        self.reset()

    def reset(self):
        n = self.thr32.size
        self.err = np.zeros(4)
        self.tp, self.fp, self.fn = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.loss, self.batches = 0.0, 0

    def record(self, y_dict, pred, mask, epoch, loss=None):
        if self.model_type == "regressor":
            for k, (key, col) in enumerate(TERMS):
                m = _np(mask[key])[:, 0].astype(np.float64)
                y = _np(y_dict[key])[:, col].astype(np.float32).astype(np.float64)
                p = _np(pred[key])[:, col].astype(np.float32).astype(np.float64)
                live = m != 0
                self.err[k] += float(np.sum(m[live] * (y[live] - p[live]) ** 2))
                if epoch == 0:
                    self.norm[k] += float(np.sum(m[live] * y[live] ** 2))
            counted = _np(mask["grain"])[:, 0] > 0
            score = _np(pred["grain_area"]).reshape(-1).astype(np.float32)
            label = _np(y_dict["grain_event"]).reshape(-1)
            pos = score[:, None] < self.thr32[None, :]
            neg = score[:, None] >= self.thr32[None, :]
        else:
            label = _np(y_dict["edge_event"]).reshape(-1)
            counted = label > -1
            z = _np(pred["edge_event"]).reshape(-1).astype(np.float32).astype(np.float64)
            with np.errstate(over="ignore"):
                score = (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
            pos = score[:, None] > self.thr32[None, :]
            neg = score[:, None] <= self.thr32[None, :]
        one, zero = ((label == 1) & counted)[:, None], ((label == 0) & counted)[:, None]
        self.tp += (one & pos).sum(0)
        self.fp += (zero & pos).sum(0)
        self.fn += (one & neg).sum(0)
        if loss is not None:
            self.loss += float(loss)
            self.batches += 1

    def errors(self):
        """(x_err, y_err, s_err, v_err) of epoch_summary (metrics.py:91-94)."""
        e, n = self.err, self.norm
        return tuple(100 * math.sqrt(float(e[k]) / float(n[k])) for k in (2, 3, 0, 1))

    def lists(self):
        """(test_auc, plist, rlist) in the reference's tensor arithmetic."""
        area, left, ps, rs = 0, 0, [], []
        for t, f, n in zip(self.tp, self.fp, self.fn):
            t, f, n = torch.tensor(int(t)), torch.tensor(int(f)), torch.tensor(int(n))
            p = r = -1
            if t + f > 0 and t + n > 0:
                p, r = t / (t + f), t / (t + n)
                area += (r - left) * p
                left = r
            ps.append(float(p))
            rs.append(float(r))
        return area, ps, rs

    def mean_loss(self):
        return self.loss / self.batches


class HostLoop:
    """The COST model of the reference's metric on device tensors (tools/eval_epoch_ab.py, arm (a)): per record one
    `float(torch.sum(...))` -- a host synchronisation -- per error term (and per norm term in epoch 0) and a boolean
    selection of the counted scores and labels (its size is data: another synchronisation); per summary TP / FP / FN per
    threshold with Python's built-in `sum` over a boolean tensor, element by element through the interpreter.  The values
    are the restatement's (tests compare them); what this class is for is what they cost when obtained that way."""

    def __init__(self, model_type):
        self.model_type = model_type
        self.err, self.norm = [0.0] * 4, [0.0] * 4
        self.scores, self.labels = [], []

    def record(self, y_dict, pred, mask, epoch):
        if self.model_type == "regressor":
            for k, (key, col) in enumerate(TERMS):
                m, y, p = mask[key][:, 0], y_dict[key][:, col], pred[key][:, col]
                self.err[k] += float(torch.sum(torch.where(m != 0, m * (y - p) ** 2, torch.zeros_like(y))))
                if epoch == 0:
                    self.norm[k] += float(torch.sum(torch.where(m != 0, m * y ** 2, torch.zeros_like(y))))
            keep = mask["grain"][:, 0] > 0
            self.scores.append(pred["grain_area"][keep])
            self.labels.append(y_dict["grain_event"][keep])
        else:
            keep = y_dict["edge_event"] > -1
            self.scores.append(pred["edge_event"][keep])
            self.labels.append(y_dict["edge_event"][keep])

    def summary(self):
        """-> (tp, fp, fn) lists of ints; the error sums are reset, the selections dropped."""
        score, label = torch.cat(self.scores), torch.cat(self.labels)
        if self.model_type == "classifier":
            score = torch.sigmoid(score)
        tp, fp, fn = [], [], []
        for t in thresholds(self.model_type):
            pos, neg = (score < t, score >= t) if self.model_type == "regressor" else (score > t, score <= t)
            tp.append(int(sum((label == 1) & pos)))
            fp.append(int(sum((label == 0) & pos)))
            fn.append(int(sum((label == 1) & neg)))
        self.err = [0.0] * 4
        self.scores, self.labels = [], []
        return tp, fp, fn


def accumulator(metric):
    """(err[4], norm[4], loss, tp, fp, fn, batches) of a feature_metric's accumulator, read back."""
    host = metric.acc.cpu()
    f = host[:9].view(torch.float64).numpy().copy()
    i = host[9:].numpy().copy()
    n = len(thresholds(metric.model_type))
    return f[0:4], f[4:8], float(f[8]), i[0:n], i[MAX_THR:MAX_THR + n], i[2 * MAX_THR:2 * MAX_THR + n], int(i[3 * MAX_THR])


def rel(got, ref):
    """max |got - ref| / |ref| over the entries (0 where both are 0; inf where got is not finite)."""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    if got.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(got == ref, 0.0, np.abs(got - ref) / np.abs(ref))
    r[~np.isfinite(got)] = np.inf
    return float(r.max())


def assert_matches(metric, ref, sum_rtol, what=""):
    """Counts EQUAL, sums within sum_rtol relative of the restatement `ref`."""
    err, norm, loss, tp, fp, fn, batches = accumulator(metric)
    assert np.array_equal(tp, ref.tp) and np.array_equal(fp, ref.fp) and np.array_equal(fn, ref.fn), \
        (what, tp, ref.tp, fp, ref.fp, fn, ref.fn)
    e, n = rel(err, ref.err), rel(norm, ref.norm)
    print(f"{what}: err rel {e:.3e}, norm rel {n:.3e} (bound {sum_rtol:g})")
    assert e <= sum_rtol and n <= sum_rtol, (what, e, n, err, ref.err, norm, ref.norm)
    assert batches == ref.batches, (what, batches, ref.batches)
    if ref.batches:
        assert rel(loss, ref.loss) <= sum_rtol, (what, loss, ref.loss)


def golden_batches(d, prefix=""):
    """[[batch dict, ...] per epoch] of a golden file."""
    out = []
    for e, nb in enumerate(np.atleast_1d(d[prefix + "n_batches"])):
        tags = [f"{prefix}e{e}b{b}_" for b in range(int(nb))]
        out.append([{k[len(tag):]: d[k] for k in d.files if k.startswith(tag)} for tag in tags])
    return out
