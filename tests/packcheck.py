"""Independent statement of the packed cell layout (graingraphnn_amd/packing.py's module docstring): every entry of
`wp / bp / w2 / ep` written by hand at the offsets `node_layout` hands out -- imperative loops into zeroed matrices, where
the library's `packing.assemble` concatenates blocks.  tests/test_packing_layout.py holds `packing.pack_cell` and
`packing.pack_conv` to these BIT FOR BIT (`torch.equal`): both sides form the key-free score coefficients from the same
float64 expressions in the same order and round each to fp32 once, in the same process (one float64 BLAS), so no tolerance
is needed.
"""
import math

import torch

from graingraphnn_amd.packing import (C, EDGE_TYPES, GATES_DEC, GATES_ENC, NODE_TYPES, U4, _conv, node_layout,
                                      roundup4)


def seeded_cell(F, layer_size, seed):
    """A HeteroPGCLSTM with every parameter (weights, Linear biases, gate biases) drawn uniformly from (-1, 1)."""
    from graingraphnn_amd.modules import HeteroPGCLSTM
    cell = HeteroPGCLSTM(dict(F), layer_size, (list(NODE_TYPES), [tuple(et) for et in EDGE_TYPES]))
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in cell.parameters():
            p.copy_(torch.rand(p.shape, generator=gen) * 2 - 1)
    return cell


def seeded_conv(F_src, F_dst, k2, seed):
    from graingraphnn_amd.modules import PeriodConv
    conv = PeriodConv((F_src + k2, F_dst + k2), C)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in conv.parameters():
            p.copy_(torch.rand(p.shape, generator=gen) * 2 - 1)
    return conv


@torch.no_grad()
def reference_pack(cell, in_channels, encoder, live=NODE_TYPES, edge_types=EDGE_TYPES):
    """-> (layout, wp, bp, ep, w2) as `PackedCell` holds them, entry by entry."""
    gates = GATES_ENC if encoder else GATES_DEC
    G = len(gates)
    k2 = 0 if encoder else C
    some = _conv(cell, "i", edge_types[0]).lin_key.weight
    dev, dt = some.device, torch.float32
    F_of = dict(in_channels)
    # encoder: the sweep forms the values from the edge records (no value columns in the projection)
    enc_mfma = encoder and all(F <= 11 for F in in_channels.values())
    layout = {nt: node_layout(nt, in_channels[nt], G, edge_types, nt in live, not encoder, not enc_mfma, tuple(live))
              for nt in NODE_TYPES}
    wp, bp, w2, ep = {}, {}, {}, {}

    def put(dst_w, dst_b, row0, F, Fp, weight, bias, zero_xyz=False):
        """weight: [n, F + 96] in the reference's input order [x | h] -> n rows of the packed matrix
        from row0 on (input order [x, pad to Fp | h]); bias is ADDED to the packed bias."""
        w = weight.detach().to(dt)
        n = w.size(0)
        blk = dst_w[row0:row0 + n]
        blk[:, :F] += w[:, :F]
        if zero_xyz:
            blk[:, :3] = 0.0
        if k2:
            blk[:, Fp:Fp + C] += w[:, F:F + C]
        dst_b[row0:row0 + n] += bias.detach().to(dt)

    scale = 1.0 / math.sqrt(C)  # periodGATconv.py:226
    for nt in NODE_TYPES:
        lay = layout[nt]
        F, Fp = lay.F, lay.Fp
        W = torch.zeros(lay.ncols, Fp + k2, dtype=dt, device=dev)
        B = torch.zeros(lay.ncols, dtype=dt, device=dev)
        for et in lay.src_ets if not enc_mfma else ():
            for g, gate in enumerate(gates):
                conv = _conv(cell, gate, et)
                put(W, B, lay.v_off[et] + g * C, F, Fp, conv.lin_value.weight, conv.lin_value.bias, True)
        for et in lay.dst_ets:
            Fs = F_of[et[0]]
            for g, gate in enumerate(gates):
                conv = _conv(cell, gate, et)
                wq, bq = conv.lin_query.weight.detach().double(), conv.lin_query.bias.detach().double()
                wk, bk = conv.lin_key.weight.detach().double(), conv.lin_key.bias.detach().double()
                we = conv.lin_edge.weight.detach().double()[:, 0]
                if not k2:  # encoder: both sides see the bare feature row
                    wq, wk = wq[:, :F], wk[:, :Fs]
                M, mb = (wk.t() @ wq) * scale, (wk.t() @ bq) * scale         # [Fs (+96), F (+96)], [Fs (+96)]
                tail_w = torch.zeros(U4, wq.size(1), dtype=torch.float64, device=dev)
                tail_b = torch.zeros(U4, dtype=torch.float64, device=dev)
                tail_w[:Fs], tail_b[:Fs] = M[:Fs], mb[:Fs]
                tail_w[12], tail_b[12] = (bk @ wq) * scale, (bk @ bq) * scale
                tail_w[13], tail_b[13] = (we @ wq) * scale, (we @ bq) * scale
                put(W, B, lay.u4_off[et] + g * U4, F, Fp, tail_w, tail_b)
                if k2:
                    put(W, B, lay.u_off[et] + g * C, F, Fp, M[Fs:], mb[Fs:])
        for g, gate in enumerate(gates if lay.live else ()):
            row0 = lay.s_off + g * C
            for et in lay.dst_ets:  # HeteroConv sums the outputs -> sum the skip weights
                conv = _conv(cell, gate, et)
                put(W, B, row0, F, Fp, conv.lin_skip.weight, conv.lin_skip.bias)
            B[row0:row0 + C] += getattr(cell, "b_" + gate)[nt].detach().to(dt).view(-1)
        wp[nt], bp[nt] = W.contiguous(), B.contiguous()

        n_in = len(lay.dst_ets)
        W2 = torch.zeros(G, C, max(lay.Ka, 4), dtype=dt, device=dev)
        for d, et in enumerate(lay.dst_ets):
            for g, gate in enumerate(gates):
                conv = _conv(cell, gate, et)
                W2[g, :, d * C:(d + 1) * C] = conv.lin_l2.weight.detach().to(dt)
                W2[g, :, n_in * C + 2 * d] = conv.lin_l2.bias.detach().to(dt)
                W2[g, :, n_in * C + 2 * d + 1] = conv.lin_edge.weight.detach().to(dt)[:, 0]
        w2[nt] = W2.contiguous()

    for et in edge_types:
        et = tuple(et)
        if not layout[et[-1]].live:
            continue
        E = torch.zeros(G, 3, C, dtype=dt, device=dev)
        for g, gate in enumerate(gates):
            E[g] = _conv(cell, gate, et).lin_value.weight.detach().to(dt)[:, 0:3].t()
        ep[et] = E.contiguous()
    return layout, wp, bp, ep, w2


@torch.no_grad()
def reference_pack_conv(conv, F_src, F_dst, k2):
    """`packing.pack_conv`'s six outputs with the score coefficients written out in place."""
    dt = torch.float32
    dev = conv.lin_key.weight.device

    def pack(weight, F, zero_xyz):
        """[n, F (+96)] reference input order -> [n, roundup4(F) + k2]."""
        Fp = roundup4(F)
        w = weight.detach().to(dt)
        out = torch.zeros(w.size(0), Fp + k2, dtype=dt, device=dev)
        out[:, :F] = w[:, :F]
        if zero_xyz:
            out[:, :3] = 0.0
        if k2:
            out[:, Fp:Fp + C] = w[:, F:F + C]
        return out

    wp_src = pack(conv.lin_value.weight, F_src, True)
    bp_src = conv.lin_value.bias.detach().to(dt)
    scale = 1.0 / math.sqrt(C)
    wq, bq = conv.lin_query.weight.detach().double(), conv.lin_query.bias.detach().double()
    wk, bk = conv.lin_key.weight.detach().double(), conv.lin_key.bias.detach().double()
    we = conv.lin_edge.weight.detach().double()[:, 0]
    if not k2:
        wq, wk = wq[:, :F_dst], wk[:, :F_src]
    M, mb = (wk.t() @ wq) * scale, (wk.t() @ bq) * scale
    tail_w = torch.zeros(U4, wq.size(1), dtype=torch.float64, device=dev)
    tail_b = torch.zeros(U4, dtype=torch.float64, device=dev)
    tail_w[:F_src], tail_b[:F_src] = M[:F_src], mb[:F_src]
    tail_w[12], tail_b[12] = (bk @ wq) * scale, (bk @ bq) * scale
    tail_w[13], tail_b[13] = (we @ wq) * scale, (we @ bq) * scale
    uh_w = M[F_src:] if k2 else torch.zeros(C, wq.size(1), dtype=torch.float64, device=dev)
    uh_b = mb[F_src:] if k2 else torch.zeros(C, dtype=torch.float64, device=dev)
    wp_dst = torch.cat([pack(uh_w, F_dst, False), pack(conv.lin_skip.weight, F_dst, False),
                        pack(tail_w, F_dst, False),
                        torch.zeros(C - U4, roundup4(F_dst) + k2, dtype=dt, device=dev)])
    bp_dst = torch.cat([uh_b.to(dt), conv.lin_skip.bias.detach().to(dt), tail_b.to(dt),
                        torch.zeros(C - U4, dtype=dt, device=dev)])
    ep = conv.lin_value.weight.detach().to(dt)[:, 0:3].t().reshape(1, 3, C).contiguous()
    w2 = torch.zeros(1, C, 100, dtype=dt, device=dev)
    w2[0, :, :C] = conv.lin_l2.weight.detach().to(dt)
    w2[0, :, C] = conv.lin_l2.bias.detach().to(dt)
    w2[0, :, C + 1] = conv.lin_edge.weight.detach().to(dt)[:, 0]
    return (wp_src.contiguous(), bp_src.contiguous(), wp_dst.contiguous(), bp_dst.contiguous(), ep, w2.contiguous())
