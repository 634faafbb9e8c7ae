"""Golden validation metrics of the UNMODIFIED reference `metrics.py` (feature_metric.record / epoch_summary,
edge_error_metric), loaded BY PATH: the repository's own top-level `metrics.py` would shadow it on sys.path.  The file
imports only torch and numpy.

Runs only where the reference checkout is available (GGNN_REFERENCE, default /root/reference); writes data only:
    python tests/golden/make_golden_metrics.py
      metrics_regressor.npz    three "epochs" (0, 1, 2) of three batches of different sizes (118/236, 200/400, 37/74 grain /
                               joint rows), ~10 % of the rows masked, grain_area uniform on [0, 1.5e-3] with some scores set
                               EXACTLY to a float32 threshold, grain_event ~20 % ones
      metrics_classifier.npz   the same structure; labels from {-100, 0, 1}; logits kept away from the thresholds (below)
      metrics_novalid.npz      one batch per model type without a single positive label: no threshold is valid
      metrics_edge_error.npz   edge_error_metric on the before / after edge lists of golden_cfg1_events.npz's cases

Per fixture with epochs: inputs `e{E}b{B}_{name}`; `acc_dicts [records, 8]` after every record in the order of ACC_KEYS;
`plist`, `rlist [epochs, n_thr]`, `test_auc [epochs]` (float32 as the reference holds it), `auc_is_int [epochs]`,
`metric_list [epochs]`, `lines` (what epoch_summary printed, one string per epoch).

Separation condition: the kernel's fp32 sigmoid may differ from torch's by an ulp, so the classifier's logits are CONSTRUCTED
so that no fp64 sigmoid lies within SEPARATION = 1e-5 (~170 fp32 ulps at 1) of one of the eleven thresholds: a logit that
does is drawn again.  None is left out; the condition is asserted here and again by every test before it compares.
"""
import contextlib
import importlib.util
import io
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("GGNN_REFERENCE", "/root/reference")
ACC_KEYS = ("grain0err", "grain1err", "joint0err", "joint1err", "grain0", "grain1", "joint0", "joint1")
REGRESSOR_THRESHOLDS = (1e-4, 2e-4, 4e-4, 6e-4, 8e-4, 1e-3)
CLASSIFIER_THRESHOLDS = tuple(1 - i / 10 for i in range(11))
SEPARATION = 1e-5
SIZES = ((118, 236), (200, 400), (37, 74))
EDGES = (708, 1200, 222)


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_metrics", os.path.join(REFERENCE, "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def separated(logits):
    """True where the fp64 sigmoid of the (float32) logit is farther than SEPARATION from every classifier threshold."""
    s = 1.0 / (1.0 + np.exp(-np.asarray(logits, np.float32).astype(np.float64)))
    return np.all(np.abs(s[:, None] - np.asarray(CLASSIFIER_THRESHOLDS)[None, :]) > SEPARATION, axis=1)


def separated_logits(rs, n, scale=2.0):
    z = (scale * rs.standard_normal(n)).astype(np.float32)
    for _ in range(100):
        bad = ~separated(z)
        if not bad.any():
            return z
        z[bad] = (scale * rs.standard_normal(int(bad.sum()))).astype(np.float32)
    raise AssertionError("could not separate the logits from the thresholds")


def regressor_batch(rs, ng, nj, events=0.2):
    b = {}
    for key, n in (("grain", ng), ("joint", nj)):
        b[f"y_{key}"] = rs.uniform(-1, 1, (n, 2)).astype(np.float32)
        b[f"p_{key}"] = (b[f"y_{key}"] + 0.1 * rs.standard_normal((n, 2))).astype(np.float32)
        b[f"mask_{key}"] = (rs.uniform(size=(n, 1)) > 0.1).astype(np.float32)
    area = rs.uniform(0, 1.5e-3, ng).astype(np.float32)
    hit = rs.choice(ng, size=min(ng, 2 * len(REGRESSOR_THRESHOLDS)), replace=False)   # scores exactly ON a threshold
    area[hit] = np.asarray(REGRESSOR_THRESHOLDS, np.float32)[np.arange(hit.size) % len(REGRESSOR_THRESHOLDS)]
    b["grain_area"] = area
    b["grain_event"] = (rs.uniform(size=ng) < events).astype(np.int64)
    return b


def classifier_batch(rs, n, labels=(-100, 0, 1)):
    return {"edge_event_logit": separated_logits(rs, n), "edge_event": rs.choice(np.asarray(labels, np.int64), size=n)}


def dicts(model_type, b):
    """(y_dict, pred, mask) of torch tensors from one batch's arrays."""
    t = torch.from_numpy
    if model_type == "regressor":
        return ({"grain": t(b["y_grain"]), "joint": t(b["y_joint"]), "grain_event": t(b["grain_event"])},
                {"grain": t(b["p_grain"]), "joint": t(b["p_joint"]), "grain_area": t(b["grain_area"])},
                {"grain": t(b["mask_grain"]), "joint": t(b["mask_joint"])})
    return {"edge_event": t(b["edge_event"])}, {"edge_event": t(b["edge_event_logit"])}, {}


def run(ref, model_type, epochs):
    """epochs = [[batch, ...], ...] -> the arrays of one golden file."""
    metric = ref.feature_metric(model_type, 0)
    out = {"model_type": np.asarray(model_type), "n_epochs": np.asarray(len(epochs)),
           "n_batches": np.asarray([len(e) for e in epochs])}
    acc, plist, rlist, auc, auc_is_int, lines = [], [], [], [], [], []
    for e, batches in enumerate(epochs):
        for k, b in enumerate(batches):
            if model_type == "classifier":
                assert separated(b["edge_event_logit"]).all()
            for name, v in b.items():
                out[f"e{e}b{k}_{name}"] = v
            metric.record(*dicts(model_type, b), e)
            acc.append([float(metric.acc_dicts.get(key, 0.0)) for key in ACC_KEYS])
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            metric.epoch_summary()
        lines.append(buf.getvalue())
        plist.append(metric.plist)
        rlist.append(metric.rlist)
        auc_is_int.append(isinstance(metric.test_auc, int))
        auc.append(np.float32(float(metric.test_auc)))
    out.update(acc_dicts=np.asarray(acc, np.float64), plist=np.asarray(plist, np.float64), rlist=np.asarray(rlist, np.float64),
               test_auc=np.asarray(auc, np.float32), auc_is_int=np.asarray(auc_is_int), lines=np.asarray(lines),
               metric_list=np.asarray(metric.metric_list, np.float64))
    return out


def edge_error(ref):
    ev = np.load(os.path.join(HERE, "golden_cfg1_events.npz"))
    cases = sorted({k.split("__")[0] for k in ev.files})
    jj, jg = ("joint", "connect", "joint"), ("joint", "pull", "grain")
    got = []
    for c in cases:
        before, after = ({et: torch.from_numpy(ev[f"{c}__{side}_ei_" + "__".join(et)]) for et in (jj, jg)} for side in ("in", "out"))
        got.append(ref.edge_error_metric(before, after) + ref.edge_error_metric(after, before))
    return {"cases": np.asarray(cases), "errors": np.asarray(got, np.float64)}   # [case, (jj, jg | swapped: jj, jg)]


def main():
    ref = load_reference()
    rs = np.random.RandomState(20240607)
    reg = run(ref, "regressor", [[regressor_batch(rs, *s) for s in SIZES] for _ in range(3)])
    cls = run(ref, "classifier", [[classifier_batch(rs, n) for n in EDGES] for _ in range(3)])
    none_r = run(ref, "regressor", [[regressor_batch(rs, 37, 74, events=0.0)]])
    none_c = run(ref, "classifier", [[classifier_batch(rs, 222, labels=(-100, 0))]])
    assert (none_r["plist"] == -1).all() and (none_c["rlist"] == -1).all() and none_r["auc_is_int"].all() and none_c["auc_is_int"].all()
    novalid = {f"{tag}__{k}": v for tag, d in (("regressor", none_r), ("classifier", none_c)) for k, v in d.items()}
    for name, d in (("regressor", reg), ("classifier", cls), ("novalid", novalid), ("edge_error", edge_error(ref))):
        path = os.path.join(HERE, f"metrics_{name}.npz")
        np.savez_compressed(path, **d)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
