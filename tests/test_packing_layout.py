"""The packed cell layout has ONE definition in the library (packing.assemble, run by pack_cell on values and by
train_pack on values and on index tensors).  Here it is held bit for bit to the independent entry-by-entry statement of
tests/packcheck.py, for every layout variant the inference path takes; pack_conv to its written-out form; and the
assembly's own check against node_layout is shown to fire.  CPU only."""
import pytest
import torch

import packcheck
from graingraphnn_amd import _lib, packing

FEATURES = ({"grain": 11, "joint": 8},      # shipped
            {"grain": 12, "joint": 12},     # the encoder keeps its value rows (no record slot left for the bias)
            {"grain": 3, "joint": 3})       # nothing but the relocation columns: empty value / feature slices


@pytest.mark.parametrize("layer_size", [96, 32])
@pytest.mark.parametrize("F", FEATURES, ids=lambda F: f"g{F['grain']}j{F['joint']}")
@pytest.mark.parametrize("live", [packing.NODE_TYPES, ("joint",)], ids=["both", "joint"])
@pytest.mark.parametrize("encoder", [True, False], ids=["enc", "dec"])
def test_pack_cell_equals_the_entry_by_entry_layout(encoder, live, F, layer_size):
    cell = packcheck.seeded_cell(F, layer_size, 7 + layer_size + F["grain"])
    src = cell if layer_size == packing.C else packing.padded_cell(cell, layer_size)
    pc = packing.pack_cell(src, F, encoder, live=live)
    layout, wp, bp, ep, w2 = packcheck.reference_pack(src, F, encoder, live)
    assert pc.layout == layout
    assert list(pc.ep) == list(ep) and list(pc.wp) == list(wp) == list(pc.bp) == list(pc.w2) == list(packing.NODE_TYPES)
    for name, got, ref in (("wp", pc.wp, wp), ("bp", pc.bp, bp), ("w2", pc.w2, w2), ("ep", pc.ep, ep)):
        for k in ref:
            assert got[k].dtype == ref[k].dtype and got[k].is_contiguous(), (name, k)
            assert torch.equal(got[k], ref[k]), (name, k)
    live_nt = [nt for nt in packing.NODE_TYPES if nt in live]
    assert all(float(pc.bp[nt].abs().max()) > 0 and float(pc.wp[nt].abs().max()) > 0 for nt in live_nt)


@pytest.mark.parametrize("k2", [0, 96])
def test_pack_conv_equals_its_written_out_form(k2):
    Fs, Fd = 11, 8
    conv = packcheck.seeded_conv(Fs, Fd, k2, 3 + k2)
    got, ref = packing.pack_conv(conv, Fs, Fd, k2), packcheck.reference_pack_conv(conv, Fs, Fd, k2)
    assert len(got) == len(ref) == 6
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.dtype == b.dtype and a.is_contiguous() and torch.equal(a, b), i


def _swap_u4(lay):
    a, b = lay.dst_ets[:2]
    lay.u4_off[a], lay.u4_off[b] = lay.u4_off[b], lay.u4_off[a]


def _swap_skip_and_first_tail(lay):
    a = lay.dst_ets[0]
    lay.s_off, lay.u4_off[a] = lay.u4_off[a], lay.s_off


@pytest.mark.parametrize("swap", [_swap_u4, _swap_skip_and_first_tail])
@pytest.mark.parametrize("encoder", [True, False], ids=["enc", "dec"])
def test_assembly_refuses_a_layout_it_does_not_follow(monkeypatch, encoder, swap):
    """node_layout moves two blocks; the assembly still concatenates in its own order: it must raise, not hand back
    matrices whose rows sit where no kernel looks for them."""
    F = FEATURES[0]
    cell = packcheck.seeded_cell(F, 96, 5)
    packing.pack_cell(cell, F, encoder)
    real = packing.node_layout

    def moved(node_type, *a, **kw):
        lay = real(node_type, *a, **kw)
        if node_type == "joint":      # two incoming edge types
            swap(lay)
        return lay
    monkeypatch.setattr(packing, "node_layout", moved)
    with pytest.raises(_lib.GGNNError):
        packing.pack_cell(cell, F, encoder)
