"""ggnn_encoder_cell_values_batch: the encoder cell with the fused decoder plan's value rows as an epilogue.

GPU: h and c bit-identical to ggnn_encoder_cell_batch; the value rows within the fp32-equivalence bound of the
three-product projection (test_three_product_projection_is_fp32_equivalent) against fp64, per element; ragged tiles,
fewer than 16 rows, hub rows, 8 and 4 blocks, batches, reproducibility; rollouts with and without the epilogue.
CPU: the packed value stream decodes back to the weights."""
import numpy as np
import pytest
import torch

from helpers import EDGE_TYPES, assert_close, product_models, tt
from graingraphnn_amd import _lib, synthetic
from graingraphnn_amd.packing import C, CELL_P3_CHANNEL, DC_LO_SCALE, DC_SLICE_I16, encoder_values_stream, roundup4

DEV = "cuda"


def _decode(stream, n_blocks, F):
    """encoder_values_stream -> (W [96 n_blocks, Fp + 96] in the projection's input order, bias): hi + lo' / 2048 of
    every fragment, the h columns un-permuted, the feature slots back to x columns."""
    s = stream.view(n_blocks * 4, 7, 2, 4, 16, 8)                 # slice | nb plane kq m j (7 column tiles, 6 used)
    assert not bool(s[:, 6].any())
    s = s[:, :6]
    v = s[:, :, 0].view(torch.float16).double() + s[:, :, 1].view(torch.float16).double() / DC_LO_SCALE
    v = v.view(n_blocks, 4, 6, 4, 16, 8).permute(0, 2, 4, 1, 3, 5)  # block nb m | ks kq j
    blk = v.reshape(n_blocks * C, 128)                             # [96 rows of each block, k = 32 ks + 8 kq + j]
    Fp = roundup4(F)
    W = torch.zeros(n_blocks * C, Fp + C, dtype=torch.float64)
    W[:, Fp + torch.tensor(CELL_P3_CHANNEL)] = blk[:, :C]
    slots = blk[:, C:].reshape(-1, 4, 8)[:, :, :4].reshape(-1, 16)   # k = 8 q + j (j < 4) <-> slot 4 q + j
    assert float(blk[:, C:].reshape(-1, 4, 8)[:, :, 4:].abs().max()) == 0.0
    W[:, :F] = slots[:, :F]
    assert not bool(slots[:, F:12].any()) and not bool(slots[:, 13:].any())
    return W, slots[:, 12]


@pytest.mark.parametrize("F,n_blocks", [(8, 8), (11, 4), (12, 1), (3, 2)])
def test_value_stream_decodes_to_the_weights(F, n_blocks):
    """The packed stream (hi + lo'/2048, h columns in GGNN_CELL_P3_CHANNEL order, features in the 16 slots, bias in
    slot 12) reproduces W_v and b_v within the two-piece fp16 rounding (2^-22 relative)."""
    rs = np.random.RandomState(F + n_blocks)
    Fp = roundup4(F)
    wpv = torch.zeros(n_blocks * C, Fp + C)
    wpv[:, :F] = torch.from_numpy(rs.standard_normal((n_blocks * C, F)) * 10 ** rs.uniform(-3, 0.5, (n_blocks * C, 1)))
    wpv[:, :3] = 0.0                                               # as the decoder's value rows hold them
    wpv[:, Fp:] = torch.from_numpy(rs.standard_normal((n_blocks * C, C)) * 10 ** rs.uniform(-3, 0.5, (n_blocks * C, 1)))
    bpv = torch.from_numpy(rs.standard_normal(n_blocks * C).astype(np.float32))
    stream = encoder_values_stream(wpv, bpv, F)
    assert stream.dtype == torch.int16 and stream.numel() == 4 * n_blocks * DC_SLICE_I16
    W, b = _decode(stream, n_blocks, F)
    tol = lambda ref: 2.0 ** -21 * ref.abs() + 2.0 ** -36
    assert bool(((W - wpv.double()).abs() <= tol(wpv.double())).all())
    assert bool(((b - bpv.double()).abs() <= tol(bpv.double())).all())


def test_value_stream_refuses_weights_beyond_fp16_range():
    wpv, bpv = torch.zeros(C, 8 + C), torch.zeros(C)
    bpv[5] = 1e5                                                   # the bias rides in the stream too
    with pytest.raises(ValueError):
        encoder_values_stream(wpv, bpv, 8)
    wpv[3, 20] = float("nan")
    with pytest.raises(ValueError):
        encoder_values_stream(wpv, torch.zeros(C), 8)


# ---------------------------------------------------------------------------------------------------------------------
def _values_problem(be, rs, n_dst, ins, hub, F_dst, n_blocks):
    """An encoder-cell problem of test_hip_parity plus random value rows [96 n_blocks, Fp + 96] / bias."""
    from test_hip_parity import _enc_cell_problem
    fused = _enc_cell_problem(be, rs, n_dst, ins, hub, F_dst=F_dst)[0]
    Fp = roundup4(F_dst)
    rows = n_blocks * C
    wpv = torch.zeros(rows, Fp + C)
    wpv[:, :F_dst] = torch.from_numpy(rs.standard_normal((rows, F_dst)) * 10 ** rs.uniform(-2, 0, (rows, 1)))
    wpv[:, Fp:] = torch.from_numpy(rs.standard_normal((rows, C)) * 10 ** rs.uniform(-2, 0, (rows, 1)))
    bpv = torch.from_numpy(rs.standard_normal(rows).astype(np.float32))
    vstream = encoder_values_stream(wpv, bpv, F_dst).to(DEV)
    v_out = torch.full((n_blocks, n_dst, C), float("nan"), device=DEV)
    fresh = (*fused[:4], torch.full_like(fused[4], float("nan")), torch.full_like(fused[5], float("nan")))
    return fused, (fresh, vstream, v_out), wpv, bpv


def _check_values(prob, wpv, bpv, what):
    """Value rows against [x | h] . W^T + b in fp64 (h = the cell's own fp32 output): within 5e-7 of sum |x||w| + |b|."""
    (_, x, *_rest), _, v_out = prob
    h = prob[0][4]
    n, F = x.size(0), x.size(1)
    Fp = roundup4(F)
    xin = torch.cat([x.cpu().double(), torch.zeros(n, Fp - F, dtype=torch.float64), h.cpu().double()], 1)
    ref = xin @ wpv.double().t() + bpv.double()
    scale = xin.abs() @ wpv.double().abs().t() + bpv.double().abs()
    got = v_out.cpu().double().permute(1, 0, 2).reshape(n, -1)     # [blocks][N][96] -> [N, 96 blocks]
    err = float(((got - ref).abs() / scale).max())
    assert err < 5e-7, f"{what}: value rows {err:.2e} of sum|x||w| + |b|"
    return err


@pytest.mark.gpu
@pytest.mark.parametrize("n_dst,ins,hub,F_dst,n_blocks", [
    (20000, [(10000, 11, 60000), (20000, 8, 60000)], 0, 8, 8),   # cfg3 junctions: two incoming edge types, 8 blocks
    (10000, [(20000, 8, 60000)], 0, 11, 4),                     # cfg3 grains: one, 4 blocks
    (236, [(118, 11, 708), (236, 8, 708)], 0, 8, 8),
    (1, [(1, 11, 1)], 0, 8, 8), (5, [(9, 8, 11), (5, 8, 0)], 0, 8, 4),   # fewer than 16 rows
    (17, [(30, 12, 60)], 0, 12, 3), (67, [(30, 8, 500)], 0, 11, 4),    # ragged last tiles, surplus waves
    (50, [(70, 8, 400), (70, 11, 1300)], 37, 8, 8), (50, [(70, 11, 1300)], 900, 11, 4)])   # hub rows
@torch.no_grad()
def test_encoder_values_against_the_cell_and_fp64(n_dst, ins, hub, F_dst, n_blocks):
    """h and c bit-identical to ggnn_encoder_cell_batch on the same inputs; the value rows within the three-product
    projection's fp32-equivalence bound against fp64; two launches bit-identical."""
    from test_hip_parity import backend
    be = backend()
    if be.lib.ggnn_gemm_mode() != 1:
        pytest.skip("split GEMM kernels only")
    rs = np.random.RandomState(n_dst + 3 * hub + n_blocks)
    fused, prob, wpv, bpv = _values_problem(be, rs, n_dst, ins, hub, F_dst, n_blocks)
    be.encoder_cell_batch([fused])
    be.encoder_cell_values_batch([prob])
    cell = prob[0]
    assert torch.equal(cell[4], fused[4]) and torch.equal(cell[5], fused[5])
    _check_values(prob, wpv, bpv, f"n_dst={n_dst} blocks={n_blocks}")
    keep = [cell[4].clone(), cell[5].clone(), prob[2].clone()]
    for t in (cell[4], cell[5], prob[2]):
        t.fill_(float("nan"))
    be.encoder_cell_values_batch([prob])
    assert torch.equal(keep[0], cell[4]) and torch.equal(keep[1], cell[5]) and torch.equal(keep[2], prob[2])
    assert not be.range_exceeded(DEV)


@pytest.mark.gpu
@torch.no_grad()
def test_encoder_values_batch_of_four_equals_single_calls():
    """Four problems (two node types x two models, 8 and 4 blocks) in one launch = four single calls, bit for bit; at
    most four problems; a wrong stream or a short output buffer is refused."""
    from test_hip_parity import backend
    be = backend()
    if be.lib.ggnn_gemm_mode() != 1:
        pytest.skip("split GEMM kernels only")
    rs = np.random.RandomState(11)
    shapes = [(2086, [(1043, 11, 6258), (2086, 8, 6258)], 8, 8), (1043, [(2086, 8, 6258)], 11, 4),
              (2086, [(1043, 11, 6258), (2086, 8, 6258)], 8, 4), (1043, [(2086, 8, 6258)], 11, 4)]
    made = [_values_problem(be, rs, n, ins, 0, F, nb) for n, ins, F, nb in shapes]
    probs = [m[1] for m in made]
    be.encoder_cell_values_batch(probs)
    outs = [[p[0][4].clone(), p[0][5].clone(), p[2].clone()] for p in probs]
    for (_, p, wpv, bpv), want in zip(made, outs):
        _check_values(p, wpv, bpv, "batched")
        for t in (p[0][4], p[0][5], p[2]):
            t.fill_(float("nan"))
        be.encoder_cell_values_batch([p])
        for a, b in zip((p[0][4], p[0][5], p[2]), want):
            assert torch.equal(a, b)
    with pytest.raises(_lib.GGNNError):
        be.encoder_cell_values_batch(probs + probs[:1])
    with pytest.raises(_lib.GGNNError):
        be.encoder_cell_values_batch([(probs[0][0], probs[0][1][:-8], probs[0][2])])
    with pytest.raises(_lib.GGNNError):
        be.encoder_cell_values_batch([(probs[0][0], probs[0][1], probs[0][2][:-1])])


def _rollout_pair(x, ei, ea, steps, **kw):
    """The same rollout with the value epilogue on (default) and off (GGNN_ENC_VALUES=0): (on, off) rollouts."""
    from graingraphnn_amd import GrainRollout, engine
    from test_hip_parity import backend
    be = backend()
    default = be.encoder_values
    R, Cm = product_models(31, 1.0, DEV)
    ros = []
    try:
        for on in (True, False):
            be.encoder_values = on
            X, EI, EA = tt(x, DEV), tt(ei, DEV), tt(ea, DEV)
            ro = GrainRollout(R, Cm, X, EI, EA, 5, **kw)
            plan = [engine.value_epilogues(be, enc, dec, ro.x) for enc, dec in ro.packed.values()]
            assert all(set(p) == ({"joint", "grain"} if on else set()) for p in plan), plan
            steps(ro)
            torch.cuda.synchronize()
            ros.append(ro)
    finally:
        be.encoder_values = default
    return ros


def _assert_rollouts_agree(a, b, what):
    for k in ("joint", "grain", "grain_area", "edge_event", "edge"):
        assert_close(a.pred[k], b.pred[k], f"{what}: encoder values on vs off, {k}", 2e-5, 2e-6)
    for nt in a.x:
        assert_close(a.x[nt], b.x[nt], f"{what}: encoder values on vs off, x {nt}", 2e-5, 2e-6)


@pytest.mark.gpu
@torch.no_grad()
def test_cfg3_rollout_with_and_without_the_value_epilogue():
    """cfg3 (10 000 grains, 20 000 junctions; two streams, R + C) with the decoders' value rows from the encoder cells
    agrees with the separate projection (GGNN_ENC_VALUES=0) within the fused-vs-split tolerance."""
    from test_hip_parity import backend
    be = backend()
    if be.lib.ggnn_gemm_mode() != 1 or not be.fused_decoder or be.fused_decoder is not True:
        pytest.skip("the fused decoder plan is not the default here")
    x, ei, ea, off = synthetic.honeycomb(100, 10, 0, return_offset=True)
    a, b = _rollout_pair(x, ei, ea, lambda ro: ro.run(3), refresh_centres=True, domain_factor=10.0,
                         domain_offset=torch.from_numpy(off))
    _assert_rollouts_agree(a, b, "cfg3 run")


@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("boundary", ["periodic", "noflux"])
def test_joint_launch_rollout_with_and_without_the_value_epilogue(boundary):
    """7 200 junctions: the fused decoder plan with both models in the same launches (joint_launches), periodic and
    no-flux boundaries, run() and step_events(): the value epilogue agrees with the separate projection."""
    from test_hip_parity import backend
    be = backend()
    if be.lib.ggnn_gemm_mode() != 1 or be.fused_decoder is not True:
        pytest.skip("the fused decoder plan is not the default here")
    x, ei, ea, off = synthetic.honeycomb(60, 6, 1, return_offset=True)
    assert be.fused_decoder_min_joints <= x["joint"].shape[0] < 8000

    def steps(ro):
        assert ro.joint_launches
        ro.run(2)
        mask = {nt: np.ones((ro.x[nt].size(0), 1), np.int64) for nt in ("grain", "joint")}
        ro.enable_events(mask, area_threshold=-1.0, edge_threshold=0.999999)
        ro.step_events()
        ro.step_events()

    a, b = _rollout_pair(x, ei, ea, steps, refresh_centres=True, domain_factor=6.0, domain_offset=torch.from_numpy(off),
                         boundary=boundary)
    _assert_rollouts_agree(a, b, f"joint launches, {boundary}")
