"""The rollout step's tail -- output heads, `update`, z clamp, grain centres, edge lengths, the next forward's edge records,
the event count -- against exact restatements at its edges (tests/tailcheck.py): the HIP kernels on the GPU; on the CPU the
same problems through the torch emulator (the checks accept it, within the stated shares) and through the emulator with
one term changed (the checks reject it, each bug by name).
"""
import functools

import pytest
import torch

import tailcheck as tc
from emulator import TorchEmulatorBackend

DEV = "cuda"


def backend():
    from graingraphnn_amd.backend import default_backend
    return default_backend()


def _report(what, shares):
    if shares:
        print(f"{what}: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()) + " of the bound")


# ---------------------------------------------------------------------------------------------------------------------
# Problems: built once, shared, never changed (the runners copy what a call writes)
# ---------------------------------------------------------------------------------------------------------------------
REG_CASES = [(nj, ng, f, "plain") for nj, ng in tc.REG_SHAPES for f in (11, 6)] \
    + [(17, 15, f, case) for case in tc.FLAG_CASES[1:] for f in (11, 6)]
EDGE_CASES = [(counts, f) for counts in tc.EDGE_COUNTS for f in (11, 12)]
EVENT_CASES = [(n, E, "mixed", None, None) for n, E in tc.EVENT_SHAPES] \
    + [(64, 193, "mixed", None, 1), (65, 190, "all", None, None), (63, 193, "none", None, None),
       (64, 193, "mixed", 193 - 37, None), (300, 212, "mixed", 0, None)]


def _id(case):
    return "-".join("x".join(map(str, c)) if isinstance(c, tuple) else str(c) for c in case)


@functools.lru_cache(maxsize=None)
def _reg(case):
    return tc.regressor_problem(*case)


@functools.lru_cache(maxsize=None)
def _cls(case):
    return tc.classifier_problem(case)


@functools.lru_cache(maxsize=None)
def _edges(case):
    return tc.edge_problem(*case)


@functools.lru_cache(maxsize=None)
def _centres(case):
    P = tc.centres_problem(*case)
    return P, tc.centres_reference(P)


@functools.lru_cache(maxsize=None)
def _events(case):
    return tc.events_problem(*case)


# ---------------------------------------------------------------------------------------------------------------------
# The stages, for any backend: (failures, shares)
# ---------------------------------------------------------------------------------------------------------------------
def regressor_stage(be, dev, case):
    """Heads alone, heads + update in two launches and in one; the fused launch equals the separate ones bit for bit; with
    "all_above" a second call that brings grain 0 back below zmax writes 0 over the 1."""
    P = _reg(case)
    fails, shares, outs = [], {}, {}
    for mode in ("heads", "separate", "fused"):
        outs[mode] = tc.run_regressor(be, dev, P, mode)
        f, s = tc.check_regressor(P, outs[mode], mode)
        fails += [f"{mode}: {m}" for m in f]
        shares = {k: max(v, shares.get(k, 0.0)) for k, v in s.items()}
    for k in outs["fused"]:
        if not tc.same_bits(outs["fused"][k], outs["separate"][k]):
            fails.append(f"fused and separate launches differ in {k}")
    if case[3] == "all_above":
        first = outs["fused"]
        if first["flags"][1] != 1:
            fails.append("the flag case did not set flags[1]")
        state = {k: first[k] for k in ("xj_buf", "xg_buf", "flags")}
        assert tc.regressor_in_between(P, state, -0.5) == 0
        for mode in ("separate", "fused"):
            f, _ = tc.check_regressor(P, tc.run_regressor(be, dev, P, mode, state, -0.5), mode, state, -0.5)
            fails += [f"second call, {mode}: {m}" for m in f]
    return fails, shares


def edges_stage(be, dev, case, entry, flag=0, mirror=False, e_dev=False):
    P = _edges(case)
    return tc.check_edges(P, tc.run_edges(be, dev, P, entry, flag, mirror, e_dev), entry, flag, mirror)


def centres_stage(be, dev, case):
    P, ref = _centres(case)
    return tc.check_centres(P, tc.run_centres(be, dev, P), ref)


def events_stage(be, dev, case, range_word=True, traj=False):
    """With a skipped grain: also the same problem with skip_grain = -1, which counts that grain."""
    P = _events(case)
    fails, _ = tc.check_events(P, tc.run_events(be, dev, P, range_word, traj), range_word)
    if P["skip"] >= 0:
        Q = {**P, "skip": -1}
        if tc.events_reference(Q)[0] != tc.events_reference(P)[0] + 1:
            fails.append("the skipped grain is no candidate")
        fails += [f"skip_grain = -1: {m}" for m in tc.check_events(Q, tc.run_events(be, dev, Q, range_word, traj), range_word)[0]]
    return fails, {}


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", REG_CASES, ids=_id)
@torch.no_grad()
def test_regressor_heads_and_update(case):
    """ggnn_heads_regressor, ggnn_step_update and ggnn_heads_regressor_update: y within the per-element bound of fp64 (exactly
    +-1 where exp overflows or underflows), grain_area / x / flags bit-exact from the kernel's own y, sentinel columns and
    every column nobody owns untouched; joint / grain split and grid end around a workgroup edge; f = 11 and 6."""
    fails, shares = regressor_stage(backend(), DEV, case)
    _report(f"regressor {_id(case)}", shares)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("case", tc.CLS_CASES)
@torch.no_grad()
def test_classifier_heads(case):
    """ggnn_heads_classifier against the fp64 pair formulation; a list shrunk in place (*E_dev = E_cap - 37 and 0) leaves the
    outputs behind it at their NaN pre-fill; an out-of-range endpoint gives NaN in exactly that edge's three outputs."""
    P = _cls(case)
    fails, shares = tc.check_classifier(P, tc.run_classifier(backend(), DEV, P))
    _report(f"classifier {case} (E = {P['E']} of {P['E_cap']})", shares)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("entry,flag,mirror,e_dev", [("refresh", 0, False, False), ("refresh", 1, False, False),
                                                      ("prepare", 0, False, False), ("refresh_prepare", 0, True, False),
                                                      ("refresh_prepare", 1, True, False), ("refresh_prepare", 1, False, False),
                                                      ("refresh", 0, False, True), ("prepare", 1, False, True),
                                                      ("refresh_prepare", 0, True, True)])
@pytest.mark.parametrize("case", EDGE_CASES, ids=_id)
@torch.no_grad()
def test_edge_lengths_and_records(case, entry, flag, mirror, e_dev):
    """ggnn_step_refresh, ggnn_edge_prepare and ggnn_step_refresh_prepare on three edge types in one call: records bit-exact
    (min-image slots, copied features, bias and zero slots, zero padding rows, nothing behind them), lengths within 1.01 * 2^-23
    of fp64, the z clamp and the mirror exact; full, nearly full and padding-only last workgroups, an empty type in the
    middle, f_src = 8 / 11 / 12, tables shrunk in place."""
    fails, shares = edges_stage(backend(), DEV, case, entry, flag, mirror, e_dev)
    _report(f"edges {_id(case)} {entry} flag={flag} e_dev={e_dev}", shares if entry != "prepare" else {})
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("case", tc.CENTRE_CASES, ids=_id)
@torch.no_grad()
def test_grain_centres(case):
    """ggnn_grain_centres (periodic, noflux, folded by 3 and by 2): rows of 0 .. 25 and 300 junctions around the batches of
    eight, the last row ending at the last entry of col, n_grain around a workgroup; dyadic grains exact."""
    fails, shares = centres_stage(backend(), DEV, case)
    _report(f"centres {_id(case)}", shares)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("case", EVENT_CASES, ids=_id)
@torch.no_grad()
def test_event_count(case):
    """ggnn_detect_events: exact counts with values on and one ulp beside the thresholds, NaN, live words 0 / -1 / 2, src >=
    dst, a skipped grain, all / no candidates, a shrunk list; with and without a range word; ggnn_detect_events_traj with one
    trajectory gives the same totals."""
    be = backend()
    for kw in ({}, {"range_word": False}) + (() if case[4] is not None else ({"traj": True},)):
        fails, _ = events_stage(be, DEV, case, **kw)
        assert not fails, (kw, fails)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the problems' decision margins, the checks accept the emulator, and reject one-term bugs by name
# ---------------------------------------------------------------------------------------------------------------------
def test_no_decision_operand_lies_between_exact_and_the_margin():
    for case in REG_CASES:
        assert tc.regressor_in_between(_reg(case)) == 0, case
    for case in EDGE_CASES:
        assert tc.edges_in_between(_edges(case)) == 0, case
    for case in tc.CENTRE_CASES:
        assert _centres(case)[1][3] == 0, case


@pytest.mark.parametrize("case", REG_CASES, ids=_id)
@torch.no_grad()
def test_regressor_check_accepts_the_emulator(case):
    fails, shares = regressor_stage(TorchEmulatorBackend(), "cpu", case)
    _report(f"regressor {_id(case)}: fp32 restatement", shares)
    assert not fails, fails
    assert max(shares.values()) <= 0.5, shares
    order = tc.kernel_order_share(_reg(case))          # the kernel's own summation order, every operation rounded once
    print(f"regressor {_id(case)}: kernel-order sum at {order:.3f} of delta")
    assert order <= 0.5, order


@pytest.mark.parametrize("case", tc.CLS_CASES)
@torch.no_grad()
def test_classifier_check_accepts_the_emulator(case):
    P = _cls(case)
    fails, shares = tc.check_classifier(P, tc.run_classifier(TorchEmulatorBackend(), "cpu", P))
    _report(f"classifier {case}: fp32 restatement", shares)
    assert not fails, fails
    assert max(shares.values()) <= 0.5, shares


@pytest.mark.parametrize("entry,flag,mirror,e_dev", [("refresh", 1, False, False), ("prepare", 0, False, True),
                                                      ("refresh_prepare", 0, True, False), ("refresh_prepare", 1, True, True)])
@pytest.mark.parametrize("case", EDGE_CASES, ids=_id)
@torch.no_grad()
def test_edge_check_accepts_the_emulator(case, entry, flag, mirror, e_dev):
    for be in (TorchEmulatorBackend(), tc.MutantBackend(None)):
        fails, shares = edges_stage(be, "cpu", case, entry, flag, mirror, e_dev)
        assert not fails, fails
        assert shares["length"] <= 1.0
    _report(f"edges {_id(case)} {entry}: fp32 restatement", shares if entry != "prepare" else {})


@pytest.mark.parametrize("case", tc.CENTRE_CASES, ids=_id)
@torch.no_grad()
def test_centre_check_accepts_the_emulator(case):
    fails, shares = centres_stage(TorchEmulatorBackend(), "cpu", case)
    _report(f"centres {_id(case)}: fp32 restatement", shares)
    assert not fails, fails
    assert shares["centre"] <= 0.5, shares


@pytest.mark.parametrize("case", EVENT_CASES, ids=_id)
@torch.no_grad()
def test_event_check_accepts_the_emulator(case):
    for be in (TorchEmulatorBackend(), tc.MutantBackend(None)):
        fails, _ = events_stage(be, "cpu", case)
        assert not fails, fails


# the problem on which each one-term bug must be seen
_R, _E256, _E253 = (17, 15, 11, "plain"), ((256, 1, 509), 11), ((253, 0, 254), 12)
BUG_STAGES = {
    "times_0.2f": lambda be: regressor_stage(be, "cpu", _R),
    "area_from_updated_area": lambda be: regressor_stage(be, "cpu", _R),
    "flag_by_last_grain": lambda be: regressor_stage(be, "cpu", (17, 15, 6, "zero_below_others_above")),
    "wrap_ge": lambda be: edges_stage(be, "cpu", _E253, "prepare"),
    "two_shifts": lambda be: edges_stage(be, "cpu", _E253, "refresh"),
    "chain_against_first_vertex": lambda be: centres_stage(be, "cpu", ("periodic", 255)),
    "inbound_shift_per_vertex": lambda be: centres_stage(be, "cpu", ("periodic", 256)),
    "row_of_9_read_as_8": lambda be: centres_stage(be, "cpu", ("periodic", 257)),
    "last_edge_of_workgroup_dropped": lambda be: edges_stage(be, "cpu", _E256, "prepare"),
    "stale_length_in_record": lambda be: edges_stage(be, "cpu", _E256, "refresh_prepare"),
    "src_le_dst_counted": lambda be: events_stage(be, "cpu", EVENT_CASES[1]),
    "area_le_threshold_counted": lambda be: events_stage(be, "cpu", EVENT_CASES[2]),
    "clamp_skips_grains": lambda be: edges_stage(be, "cpu", _E253, "refresh_prepare", 1, True),
}


@pytest.mark.parametrize("bug", tc.BUGS)
@torch.no_grad()
def test_checks_reject_a_one_term_bug(bug):
    """The same stage passes with the unchanged emulator methods and fails with the one changed term."""
    fails, _ = BUG_STAGES[bug](tc.MutantBackend(None))
    assert not fails, fails
    fails, _ = BUG_STAGES[bug](tc.MutantBackend(bug))
    print(f"{bug}: {fails}")
    assert fails, bug
