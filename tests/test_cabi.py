"""The C-ABI library loads and exports every symbol include/ggnn.h declares (and none of those ABI 26 removed); host-side
argument validation works without a GPU (no kernel is launched here)."""
import ctypes
import os
import re

import pytest

from helpers import ROOT
from graingraphnn_amd import _lib


def header_symbols():
    src = open(os.path.join(ROOT, "include", "ggnn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ggnn_[a-z_0-9]+)\s*\(", src)))


def test_header_and_binding_agree():
    assert header_symbols() == sorted(_lib.EXPORTED_SYMBOLS)


def test_library_exports_every_declared_symbol():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym in header_symbols():
        assert hasattr(lib, sym), sym


# What ABI 26 removed: the single-problem forms of the *_batch entry points and the older signatures of merged operations.
REMOVED_IN_ABI_26 = (
    "ggnn_build_csr", "ggnn_build_csr_masked_batch", "ggnn_project", "ggnn_period_gat_aggregate", "ggnn_lstm_epilogue",
    "ggnn_lstm_train_forward", "ggnn_lstm_train_backward", "ggnn_pack_weights", "ggnn_pack_weights_backward",
    "ggnn_detect_events_n", "ggnn_detect_events_skip", "ggnn_heads_classifier_n", "ggnn_grain_centres_bc",
)


def test_library_exports_no_removed_symbol():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym in REMOVED_IN_ABI_26:
        assert not hasattr(lib, sym), sym
        assert sym not in _lib.EXPORTED_SYMBOLS and sym not in header_symbols(), sym


def test_version_and_host_only_queries():
    lib = _lib.load()
    assert lib.ggnn_version() == _lib.GGNN_ABI_VERSION == 26
    assert lib.ggnn_error_string(0) == b"ok"
    assert b"invalid" in lib.ggnn_error_string(-1)
    assert lib.ggnn_csr_workspace_bytes(60000, 20000) == (2 * 20000 + 2) * 4
    # decoder-sized scratch of one model forward at cfg3 (DESIGN.md "data layout")
    floats = 20000 * 2688 + 10000 * 1536 + 20000 * 784 + 10000 * 400 + 4 * 30000 * 96 + 20000 * 8 + 3 * 60000
    assert lib.ggnn_workspace_bytes(10000, 20000, 60000) == 4 * floats


def test_argument_validation_returns_einval_without_launching():
    lib = _lib.load()
    assert lib.ggnn_project_batch(None, 1, None) == -1
    assert lib.ggnn_project_batch((_lib.ProjectArgs * 1)(), 1, None) == -1
    assert lib.ggnn_lstm_epilogue_batch(None, 1, None) == -1
    assert lib.ggnn_period_gat_aggregate_batch((_lib.AggregateArgs * 1)(), 1, None) == -1
    assert lib.ggnn_lstm_epilogue_batch((_lib.EpilogueArgs * 1)(), 1, None) == -1
    assert lib.ggnn_period_gat_aggregate_batch(None, 1, None) == -1
    assert lib.ggnn_period_gat_aggregate_batch((_lib.AggregateArgs * 3)(), 4, None) == -1
    assert lib.ggnn_period_gat_aggregate_backward(None, None) == -1
    b = _lib.AggregateBwdArgs()
    assert lib.ggnn_period_gat_aggregate_backward(ctypes.byref(b), None) == -1
    assert lib.ggnn_aggregate_bwd_partials(20000) == 768 and lib.ggnn_aggregate_bwd_partials(5) == 2
    assert lib.ggnn_build_csr_batch(None, None, 1, None) == -1
    c = (_lib.CsrArgs * 1)()
    c[0].E, c[0].n_src, c[0].n_dst = 5, 3, 0      # (the refused single build's operands: no tables, no destination rows)
    assert lib.ggnn_build_csr_batch(c, None, 1, None) == -1
    assert lib.ggnn_build_csr_batch(c, (_lib.CsrMask * 1)(), 1, None) == -1
    assert lib.ggnn_csr_max_units(60000, 20000) == 40001
    assert lib.ggnn_edge_prepare(None, 1, None) == -1
    assert lib.ggnn_heads_regressor(None, 1, None, 1, None, 11, None, None, None, None, None, None) == -1
    assert lib.ggnn_heads_classifier(None, 1, None, 0, None, None, None, None, None, None, None, None) == -1
    assert lib.ggnn_detect_events(None, None, 1, 0.0, None, None, 0, None, 0.0, None, None, -1, None) == -1
    assert lib.ggnn_grain_centres(None, None, None, 1, 8, None, 1.0, None, 1, 11, None, _lib.BC_PERIODIC, None) == -1
    buf = (ctypes.c_float * 32)()                 # (host memory: refused before anything would be launched)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.ggnn_grain_centres(p, p, p, 1, 8, None, 1.0, p, 1, 11, None, 7, None) == -1    # no such boundary
    assert lib.ggnn_step_update(None, 1, 8, None, 1, 11, 11, None, None, 0.0, 1.0, None, None) == -1
    assert lib.ggnn_step_refresh(None, 1, 8, None, 1, 11, 1.0, None, None, 0, None) == -1
    with pytest.raises(_lib.GGNNError):
        _lib.check(-1, "demo")


@pytest.mark.parametrize("E_cap,n_dst", [(0, 1), (1, 1), (5, 3), (13, 4), (60000, 20000)])
def test_csr_carver_and_arena_size_agree(E_cap, n_dst):
    """The one place that lays out a list's CSR tables (backend._csr_tables) takes, with a take that only counts, exactly
    the words csr_arena_words sizes an arena with, every table on a 16-byte boundary -- and that is the closed formula the
    arena was sized with before it was derived from the carving."""
    from graingraphnn_amd import backend
    lib = _lib.load()
    arena, starts = backend._WordArena(), []

    def take(n):
        starts.append(arena.at)
        return arena.take(n)
    assert backend._csr_tables(lib, take, E_cap, 2, n_dst) is None
    assert len(starts) == 8 and starts[0] == 0 and all(s % 4 == 0 for s in starts) and starts == sorted(set(starts))
    r4 = lambda n: (n + 3) & ~3
    formula = 2 * r4(n_dst + 1) + 3 * r4(max(E_cap, 1)) + 8 * lib.ggnn_csr_max_units(E_cap, n_dst) + 4 \
        + r4(lib.ggnn_csr_workspace_bytes(E_cap, n_dst) // 4 + 1)
    assert arena.at == backend.HipBackend().csr_arena_words(E_cap, n_dst) == formula


def test_struct_sizes_match_the_header():
    """ctypes mirrors of the POD argument blocks (natural alignment, no packing)."""
    assert ctypes.sizeof(_lib.AggregateArgs) == 8 * 8 + 7 * 8 + 8 * 4
    assert ctypes.sizeof(_lib.AggregateBwdArgs) == 18 * 8 + 8 * 8 + 8 * 4
    assert ctypes.sizeof(_lib.PrepareEdge) == 7 * 8 + 4 * 8 + 8     # (+ E_dev)
    assert ctypes.sizeof(_lib.EpilogueArgs) == 7 * 8 + 2 * 8 + 4 * 4 + 8 + 8 + 2 * 4
    assert ctypes.sizeof(_lib.RefreshEdge) == 4 * 8 + 5 * 8 + 8    # (+ E_dev)
