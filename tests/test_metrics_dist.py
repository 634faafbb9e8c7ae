"""feature_metric.reduce() over two gloo ranks (CPU): each rank records half of the batches; after reduce() every rank's
accumulator holds what one process recording all batches holds -- counts equal, fp64 sums within 1e-10 relative (the same
terms in another order: n 2^-53 with n <= 1e5, times ten).  Two epochs: the norms, reduced in epoch 0, are not summed again."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import metriccheck as mc
from graingraphnn_amd.metrics import feature_metric

N_BATCHES = 4


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _batches(model_type, epoch):
    rs = np.random.RandomState(40 + epoch + (10 if model_type == "classifier" else 0))
    if model_type == "regressor":
        return [mc.regressor_batch(rs, 50 + 17 * k, 100 + 31 * k) for k in range(N_BATCHES)]
    return [mc.classifier_batch(rs, 300 + 77 * k) for k in range(N_BATCHES)]


def _record_epochs(model_type, take, reduce):
    """Two epochs; `take(k)` selects the batches this process records.  -> the accumulator before each summary."""
    metric, out = feature_metric(model_type, 0), []
    for epoch in (0, 1):
        for k, b in enumerate(_batches(model_type, epoch)):
            if take(k):
                metric.record(*mc.dicts(model_type, b), epoch, loss=torch.tensor(float(k + 1)))
        if reduce:
            metric.reduce()
        out.append(metric.acc.clone())
        metric.epoch_summary()
    return out


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = {mt: _record_epochs(mt, lambda k: k % world == rank, True) for mt in ("regressor", "classifier")}
    torch.save(res, f"{out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_reduce_equals_one_process(tmp_path, capsys):
    torch.set_num_threads(1)
    for mt in ("regressor", "classifier"):
        for epoch in (0, 1):
            for b in _batches(mt, epoch):
                assert mt == "regressor" or mc.separated(b["edge_event_logit"]).all()
    out = str(tmp_path / "acc.pt")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    for mt in ("regressor", "classifier"):
        want = _record_epochs(mt, lambda k: True, False)
        for rank in range(2):
            got = torch.load(f"{out}.{rank}")[mt]
            for epoch in (0, 1):
                g, w = got[epoch], want[epoch]
                assert torch.equal(g[9:], w[9:]), (mt, rank, epoch)
                assert int(w[9 + 48]) == N_BATCHES
                gf, wf = g[:9].view(torch.float64).numpy(), w[:9].view(torch.float64).numpy()
                assert mc.rel(gf, wf) <= 1e-10, (mt, rank, epoch, gf, wf)
                if mt == "regressor":
                    assert (wf[:8] > 0).all()
