"""The reference's validation metrics (metrics.py: `feature_metric`, `edge_error_metric`) with the sums kept on the device.

The reference's `record` reads four scalars back per batch (`float(torch.sum(...))`) and keeps every batch's scores and labels
for `epoch_summary`, which counts true / false positives with Python's `sum` over boolean tensors: an interpreter step (and
on a GPU a device read) per element, 3 x 11 times over.  Here `record` is ONE launch (`ggnn_metric_record`) that adds the batch
into a device accumulator, and `epoch_summary` reads the accumulator back ONCE:

    acc   int64 [58], one allocation:   words 0..8 viewed as float64: err[4] | norm[4] | loss sum
                                        words 9..57 int64: TP[16] | FP[16] | FN[16] | batches with a loss
    err / norm slots (regressor):       0 grain0 (s)   1 grain1 (v)   2 joint0 (x)   3 joint1 (y)

From the counts the precision / recall lists and the PR-AUC are formed in the reference's own arithmetic (0-dim int64 tensors
divided into float32, the AUC accumulated in float32, -1 for a threshold without a positive), so they equal the reference's
bit for bit; the error sums are fp64 sums of fp64 terms where the reference sums fp32 products.  One deliberate difference:
a row whose mask is 0 adds exactly 0 even where the prediction is not finite (0 * inf is NaN in the reference), the choice
`training.classifier_loss` makes for unlabelled edges.  On CPU tensors the same arithmetic runs as torch ops into the same
layout, so the class needs no GPU.
"""
import math

import torch

from . import _lib

N_F64, N_I64 = _lib.GGNN_METRIC_F64_SLOTS, _lib.GGNN_METRIC_I64_SLOTS
MAX_THR = _lib.GGNN_METRIC_MAX_THR
LOSS_SLOT, BATCH_SLOT = 8, 3 * MAX_THR
# metrics.py:136 (grain events: positive = area BELOW the threshold) and :188 `1 - i / intervals` (edge events: positive =
# sigmoid ABOVE it).  The comparisons run in float32 against the threshold rounded to float32, as torch's do.
REGRESSOR_THRESHOLDS = (1e-4, 2e-4, 4e-4, 6e-4, 8e-4, 1e-3)
CLASSIFIER_THRESHOLDS = tuple(1 - i / 10 for i in range(11))
TERMS = (("grain", 0), ("grain", 1), ("joint", 0), ("joint", 1))   # the order of metrics.py:46-49 = the slots


def thresholds_of(model_type):
    return REGRESSOR_THRESHOLDS if model_type == "regressor" else CLASSIFIER_THRESHOLDS


def _row_mask(m):
    """mask[key][:, 0] as float32, one value per row (a view where the mask already is float32)."""
    m = m[:, 0] if m.dim() == 2 else m
    return m if m.dtype == torch.float32 else m.to(torch.float32)


def _f32(t):
    return t if t.dtype == torch.float32 else t.to(torch.float32)


def record_torch(acc, model_type, y_dict, pred, mask, with_norm, loss=None):
    """`ggnn_metric_record` as torch ops (any device): the same fp64 terms and integer counts into the same layout."""
    f64, i64 = acc[:N_F64].view(torch.float64), acc[N_F64:]
    thr = torch.tensor(thresholds_of(model_type), dtype=torch.float32, device=acc.device)
    if model_type == "regressor":
        for k, (key, col) in enumerate(TERMS):
            m = _row_mask(mask[key])
            live = m != 0
            y = _f32(y_dict[key])[:, col].to(torch.float64)
            p = _f32(pred[key])[:, col].to(torch.float64)
            zero = torch.zeros((), dtype=torch.float64, device=acc.device)
            w = m.to(torch.float64)
            f64[k] += torch.where(live, w * (y - p) ** 2, zero).sum()
            if with_norm:
                f64[4 + k] += torch.where(live, w * y ** 2, zero).sum()
        score, label = _f32(pred["grain_area"]).reshape(-1), y_dict["grain_event"].reshape(-1)
        counted = _row_mask(mask["grain"]) > 0
        pos, neg = score[:, None] < thr[None, :], score[:, None] >= thr[None, :]
    else:
        label = y_dict["edge_event"].reshape(-1)
        score = torch.sigmoid(_f32(pred["edge_event"]).reshape(-1))
        counted = label > -1
        pos, neg = score[:, None] > thr[None, :], score[:, None] <= thr[None, :]
    one, zero_ = ((label == 1) & counted)[:, None], ((label == 0) & counted)[:, None]
    n = thr.numel()
    i64[0:n] += (one & pos).sum(0)
    i64[MAX_THR:MAX_THR + n] += (zero_ & pos).sum(0)
    i64[2 * MAX_THR:2 * MAX_THR + n] += (one & neg).sum(0)
    if loss is not None:
        f64[LOSS_SLOT] += loss.detach().to(device=acc.device, dtype=torch.float64).reshape(())
        i64[BATCH_SLOT] += 1


def pr_auc(tp, fp, fn):
    """The precision / recall lists and the PR-AUC of metrics.py:124-217 from the counts, in the reference's arithmetic.
    There TP, FP and FN are 0-dim int64 tensors (Python's `sum` over a boolean tensor), their quotients float32 tensors, and
    the area a float32 tensor -- or the integer 0 where no threshold is valid.  A threshold is valid with TP + FP > 0 and
    TP + FN > 0; an invalid one is listed as -1 and does not move the left bound of the next recall step.  (Over an EMPTY
    selection the reference's sums are the integer 0: no valid threshold either way.)"""
    area, left = 0, 0
    precisions, recalls = [], []
    for t, f, n in zip(tp, fp, fn):
        t, f, n = (torch.tensor(int(v), dtype=torch.int64) for v in (t, f, n))
        precision = recall = -1
        if t + f > 0 and t + n > 0:
            precision, recall = t / (t + f), t / (t + n)
            area += (recall - left) * precision
            left = recall
        precisions.append(precision)
        recalls.append(recall)
    return area, precisions, recalls


class feature_metric:
    """Drop-in for the reference's `metrics.feature_metric` (train.py:95, 118, 130, 171, 181, 189; dist_train.py likewise).

        metric = feature_metric('regressor', model_id)
        for batch in loader:  metric.record(y_dict, pred, mask, epoch, loss=loss)     # one launch, no synchronisation
        metric.epoch_summary()        # ONE read-back; prints the reference's lines; -> plist, rlist, test_auc, metric_list
        metric.mean_loss()            # the epoch's validation loss: sum of the recorded losses / their number

    The accumulator lives on the device of the first recorded batch.  `epoch_summary` resets what the reference resets (the
    error sums, the counts) and the loss sum; the norms of epoch 0 stay."""

    def __init__(self, model_type, model_id):
        if model_type not in ("regressor", "classifier"):
            raise ValueError("model_type must be 'regressor' or 'classifier'")
        self.model_type, self.model_id = model_type, model_id
        self.metric_list = []
        self.acc = None
        self._mean_loss = float("nan")
        self._fresh = False   # records since the last summary
        self._norms_reduced = False

    # -- the accumulator ---------------------------------------------------------------
    def _accumulator(self, device):
        if self.acc is None:
            self.acc = torch.zeros(N_F64 + N_I64, dtype=torch.int64, device=device)
        elif self.acc.device != device:
            raise ValueError(f"feature_metric: the accumulator is on {self.acc.device}, the batch on {device}")
        return self.acc

    @property
    def f64(self):
        return self.acc[:N_F64].view(torch.float64)

    @property
    def i64(self):
        return self.acc[N_F64:]

    def _read(self):
        """(float64 list, int64 list) of the accumulator: the one read-back."""
        if self.acc is None:
            return [0.0] * N_F64, [0] * N_I64
        host = self.acc.cpu()
        return host[:N_F64].view(torch.float64).tolist(), host[N_F64:].tolist()

    @property
    def acc_dicts(self):
        """The reference's dictionary of running sums (a read-back: for inspection, not for the loop)."""
        f, _ = self._read()
        out = {}
        for k, (key, col) in enumerate(TERMS):
            out[f"{key}{col}err"], out[f"{key}{col}"] = f[k], f[4 + k]
        return out

    # -- record ------------------------------------------------------------------------
    @torch.no_grad()
    def record(self, y_dict, pred, mask, epoch, loss=None):
        regressor = self.model_type == "regressor"
        probe = pred["grain_area"] if regressor else pred["edge_event"]
        acc = self._accumulator(probe.device)
        self._fresh = True
        if not probe.is_cuda:
            record_torch(acc, self.model_type, y_dict, pred, mask, epoch == 0, loss)
            return
        from .backend import default_backend
        i64 = lambda t: t if t.dtype == torch.int64 else t.to(torch.int64)
        c = lambda t: t if t.is_contiguous() else t.contiguous()
        two_d = lambda t: t if t.dim() == 2 else t.reshape(t.size(0), -1)
        if loss is not None:
            loss = _f32(loss.detach())
        if regressor:
            rows = {key: _row_mask(mask[key]) for key in ("grain", "joint")}
            terms = [(c(two_d(_f32(pred[key].detach()))), c(two_d(_f32(y_dict[key]))), rows[key], col) for key, col in TERMS]
            default_backend().metric_record(acc, terms, epoch == 0, _lib.METRIC_REGRESSOR,
                                            c(_f32(pred["grain_area"].detach()).reshape(-1)),
                                            c(i64(y_dict["grain_event"]).reshape(-1)), rows["grain"],
                                            REGRESSOR_THRESHOLDS, loss)
        else:
            default_backend().metric_record(acc, [], False, _lib.METRIC_CLASSIFIER,
                                            c(_f32(pred["edge_event"].detach()).reshape(-1)),
                                            c(i64(y_dict["edge_event"]).reshape(-1)), None, CLASSIFIER_THRESHOLDS, loss)

    # -- summaries ---------------------------------------------------------------------
    def epoch_summary(self):
        f, i = self._read()
        n = len(thresholds_of(self.model_type))
        tp, fp, fn = i[0:n], i[MAX_THR:MAX_THR + n], i[2 * MAX_THR:2 * MAX_THR + n]
        if i[BATCH_SLOT]:
            self._mean_loss = f[LOSS_SLOT] / i[BATCH_SLOT]
        if self.model_type == "classifier":
            self.test_auc, self.plist, self.rlist = pr_auc(tp, fp, fn)
            self.plist = [float(v) for v in self.plist]
            self.rlist = [float(v) for v in self.rlist]
            print('edge event: precision ', self.plist, ', recall: ', self.rlist)
        else:
            # (Python floats: a zero norm -- no record of epoch 0 -- raises the reference's ZeroDivisionError)
            x_err = 100 * math.sqrt(f[2] / f[6])
            y_err = 100 * math.sqrt(f[3] / f[7])
            s_err = 100 * math.sqrt(f[0] / f[4])
            v_err = 100 * math.sqrt(f[1] / f[5])
            self.x_err, self.y_err, self.s_err, self.v_err = x_err, y_err, s_err, v_err
            print('err, joint x: %2.1f, y: %2.1f, grain s: %2.1f, v: %2.1f' % (x_err, y_err, s_err, v_err))
            self.test_auc, self.plist, self.rlist = pr_auc(tp, fp, fn)
            self.plist = [float(v) for v in self.plist]
            self.rlist = [float(v) for v in self.rlist]
            print('grain event: precision ', self.plist, ', recall: ', self.rlist)
        print('Validation AUC:{:.6f}'.format(self.test_auc))
        self.metric_list.append(float(self.test_auc))
        if self.acc is not None:   # what the reference resets (metrics.py:97-100, 109) and the epoch's loss; not the norms
            self.f64[0:4] = 0
            self.f64[LOSS_SLOT] = 0
            self.i64.zero_()
        self._fresh = False

    def summary(self):
        print('model id:', self.model_id, 'PR AUC', float(self.test_auc))

    def mean_loss(self):
        """Sum of the losses recorded in this epoch / their number: after `epoch_summary()` the value it read (no further
        read-back), before it one read-back of the running sums."""
        if self._fresh:
            f, i = self._read()
            return f[LOSS_SLOT] / i[BATCH_SLOT] if i[BATCH_SLOT] else float("nan")
        return self._mean_loss

    def reduce(self, group=None):
        """Sums the accumulators over a process group, in place on every rank: two all-reduces (the float64 words, the
        int64 words).  Call it once per epoch, before `epoch_summary()`.  The norms are only added to in epoch 0: once they
        have been reduced they are the group's and a later call leaves them alone.  (The reference does not do this -- each
        rank of dist_train.py summarises its own shard -- and the scripts never call it.)"""
        import torch.distributed as dist
        self._accumulator(self.acc.device if self.acc is not None else torch.device("cpu"))
        norms = self.f64[4:8].clone() if self._norms_reduced else None
        dist.all_reduce(self.f64, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.i64, op=dist.ReduceOp.SUM, group=group)
        if norms is not None:
            self.f64[4:8] = norms
        self._norms_reduced = True
        self._fresh = True


def edge_error_metric(data_edge_index, pred_edge_index):
    """metrics.py:221-232: per edge type, 1 - the share of the first argument's (source, destination) columns that the second
    argument also holds, for ('joint', 'connect', 'joint') and ('joint', 'pull', 'grain')."""
    def columns(ei):
        return set(map(tuple, ei.detach().cpu().numpy().T.tolist()))

    out = []
    for et in (("joint", "connect", "joint"), ("joint", "pull", "grain")):
        have, want = columns(pred_edge_index[et]), columns(data_edge_index[et])
        out.append(1 - len(want & have) / len(want))
    return tuple(out)
