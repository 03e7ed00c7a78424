"""CPU proof that the kernel-edge comparators (tests/kernel_checks.py) are
sensitive: each is fed the output of a deliberately wrong pure-torch
emulation of a plausible kernel bug and must reject it, and must accept
the correct emulation of the same inputs."""

import numpy as np
import pytest
import torch

import kernel_checks as kc

N_ROWS, DIM = 1100, 384  # one full 1024-row block + 64 rows + a 12-row tile
DTYPES = [torch.bfloat16, torch.float8_e4m3fn]


@pytest.fixture(scope="module", params=DTYPES, ids=["bf16", "fp8"])
def topk_case(request):
    # 256 queries = two 128-query passes; winners hit every structure the
    # mutants below break, and differ between query b and query b-128
    winners = [(7 * b + 3) % N_ROWS for b in range(256)]
    winners[0] = 1099       # partial last tile (rows 1088..1099)
    winners[1] = 300        # second wave's 256-row span
    winners[2] = 20         # an odd 16-row tile
    winners[3] = 1024       # first row of the second block
    index, q = kc.planted_case(N_ROWS, DIM, request.param, winners, seed=101)
    return index, q


def test_topk_correct_emulation_is_accepted(topk_case):
    index, q = topk_case
    hi, idx = kc.emulate_topk(index, q)
    stats = kc.check_topk(hi, idx, index, q)
    # the issue's construction: margin >= 0.59 over every other row
    assert stats["min_gap"] > 0.5
    assert stats["max_err_over_bound"] <= 1.0


def _mask(fn):
    return torch.tensor([fn(r) for r in range(N_ROWS)])


TOPK_MUTANTS = {
    "ignores_partial_last_tile": dict(row_mask=_mask(lambda r: r < (N_ROWS // 16) * 16)),
    "ignores_one_wave_span": dict(row_mask=_mask(lambda r: not 256 <= r < 512)),
    "ignores_odd_tiles": dict(row_mask=_mask(lambda r: (r // 16) % 2 == 0)),
    "second_pass_returns_first_pass_rows": dict(alias_second_pass=True),
}


@pytest.mark.parametrize("mutant", sorted(TOPK_MUTANTS))
def test_topk_mutants_are_rejected(topk_case, mutant):
    index, q = topk_case
    hi, idx = kc.emulate_topk(index, q, **TOPK_MUTANTS[mutant])
    with pytest.raises(AssertionError, match="got row"):
        kc.check_topk(hi, idx, index, q)


def test_topk_score_bound_is_tight(topk_case):
    """A right row with a score off by 1e-3 (50x tighter than the old
    2e-2 acceptance) must fail."""
    index, q = topk_case
    hi, idx = kc.emulate_topk(index, q)
    from aigw.ops.semcache import _unorder

    hi[5] = kc.order_float(_unorder(hi[5]) - 1e-3)
    with pytest.raises(AssertionError, match="bound"):
        kc.check_topk(hi, idx, index, q)


def test_topk_unfit_inputs_are_refused():
    """Random unit queries (top-1/top-2 gap ~0.008, some far smaller) are
    not a basis for an exact-row check unless the gap clears the margin;
    an exact duplicate row is refused unless allowed_rows covers it."""
    index = kc.unit_rows(N_ROWS, DIM, torch.bfloat16, seed=5)
    index[700] = index[40]
    q = index[[40]].clone()
    hi, idx = kc.emulate_topk(index, q)
    with pytest.raises(AssertionError, match="unfit"):
        kc.check_topk(hi, idx, index, q)
    kc.check_topk(hi, idx, index, q, allowed_rows=[{40, 700}])
    with pytest.raises(AssertionError, match="not the exact maximum"):
        kc.check_topk(hi, idx, index, q, allowed_rows=[{40, 41}])


def test_order_float_roundtrip():
    from aigw.ops.semcache import _unorder

    vals = [0.0, 1.0, -1.0, 0.2, -0.2, 1e-30, -1e-30, -1e30]
    for v in vals:
        f = float(np.float32(v))
        assert _unorder(kc.order_float(f)) == f
    ordered = sorted(vals)
    keys = [kc.order_float(v) for v in ordered]
    assert keys == sorted(keys)


# ------------------------------- GEMM --------------------------------------

GEMM_SHAPES = [(17, 65, 24), (128, 128, 32)]


@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
@pytest.mark.parametrize("bias,relu", [(True, True), (True, False), (False, True)])
def test_gemm_correct_emulation_is_accepted(m, n, k, bias, relu):
    a, bt, b = kc.gemm_inputs(m, n, k, seed=m + n + k, with_bias=bias)
    stats = kc.check_gemm(kc.emulate_gemm(a, bt, b, relu), a, bt, b, relu)
    assert stats["max_err_over_bound"] <= 1.0


@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_gemm_dropped_k_tail_is_rejected(m, n, k):
    a, bt, b = kc.gemm_inputs(m, n, k, seed=1, with_bias=False)
    a_cut = a.clone()
    a_cut[:, k - 8:] = 0  # the last 8-wide K group never loaded
    with pytest.raises(AssertionError, match="out of bound"):
        kc.check_gemm(kc.emulate_gemm(a_cut, bt, b, False), a, bt, b, False)


def test_gemm_bias_by_row_is_rejected():
    m, n, k = 128, 128, 32
    a, bt, b = kc.gemm_inputs(m, n, k, seed=2, with_bias=True)
    wrong = kc.emulate_gemm(a, bt, None, False) + b.float()[:, None]
    with pytest.raises(AssertionError, match="out of bound"):
        kc.check_gemm(wrong, a, bt, b, False)


def test_gemm_skipped_relu_on_tiled_shape_is_rejected():
    m, n, k = 128, 128, 32
    a, bt, b = kc.gemm_inputs(m, n, k, seed=3, with_bias=True)
    wrong = kc.emulate_gemm(a, bt, b, False)
    assert (wrong < 0).any()
    with pytest.raises(AssertionError, match="out of bound"):
        kc.check_gemm(wrong, a, bt, b, True)


def test_gemm_old_tolerance_scale_error_is_rejected():
    """An error of 1e-2 on one small element passed atol=5e-1; it must not
    pass the accumulation bound."""
    a, bt, b = kc.gemm_inputs(16, 64, 8, seed=4, with_bias=False)
    c = kc.emulate_gemm(a, bt, None, False)
    ref, bound = kc.gemm_reference(a, bt, None, False)
    i = int(bound.argmin())
    assert float(bound.flatten()[i]) < 1e-3
    c.view(-1)[i] += 1e-2
    with pytest.raises(AssertionError, match="out of bound"):
        kc.check_gemm(c, a, bt, None, False)


# ------------------------------ KV scorer ----------------------------------

@pytest.mark.parametrize("name", sorted(kc.kv_cases()))
def test_kv_cases_are_exact_in_fp32(name):
    """The GPU test compares assignments exactly, which is only fair if
    fp32 evaluation cannot disagree with fp64 on these inputs."""
    stats, pred = kc.kv_cases()[name]
    r32 = kc.kv_greedy_ref(stats, pred, kc.KV_WEIGHTS, np.float32)
    r64 = kc.kv_greedy_ref(stats, pred, kc.KV_WEIGHTS, np.float64)
    assert r32 == r64
    n_rep = len(stats)
    if name.startswith("identical") and n_rep > 1:
        # ties break to the lowest index: the first n_rep requests go 0,1,2..
        k = min(n_rep, len(r64))
        assert r64[:k] == list(range(k))
    if name.startswith("mixed") and n_rep > 2:
        # the zero-capacity and the full replica are never chosen, and the
        # overflow penalty is what keeps the full one out
        assert 0 not in r64 and (n_rep - 1) not in r64
        free = kc.kv_greedy_ref(stats, pred, kc.KV_WEIGHTS, np.float64, penalty=False)
        assert (n_rep - 1) in free
    if name.startswith("all_overflow") and n_rep > 1:
        assert len(set(r64)) > 1


# --------------------------------- BPE -------------------------------------

def test_bpe_case_constructions():
    """The constructed cases are what their names say (CPU-only facts the
    GPU cases rely on)."""
    from aigw.ops.bpe_ref import segment_starts

    cases = kc.bpe_cases()
    for name, total in [("total_255", 255), ("total_256", 256),
                        ("total_257", 257), ("total_512", 512),
                        ("empty_trailing_total_512", 512)]:
        assert sum(len(t) for t in cases[name]) == total
    assert len(cases["boundary_at_256"][0]) == 256
    assert len(b"thirteen byte") == 13
    for span in (64, 65):
        text = cases[f"group_span_{span}"][0]
        starts = segment_starts(text, [0])
        assert starts[:7] == [0, 5, 10, 15, 20, 25, 30] and starts[7] == span
    for n in (63, 64, 65, 128, 129):
        assert segment_starts(kc._letters(n, n), [0]) == [0]


# --------------------------- admission probe -------------------------------

def test_probe_lookup_inputs_and_allowance():
    """The native-lookup test's inputs are fit for it, and its score
    allowance is what the CPU measurement says: 4x the largest disagreement
    between the fp64 mirrored reference and a plain fp32 evaluation."""
    from aigw.ops.bpe_ref import BPERef, make_merges

    ref = BPERef(make_merges(kc.PROBE_N_MERGES, kc.PROBE_SEED))
    texts = kc.probe_lookup_texts()
    assert len(texts) == 130 and len(set(texts)) == 130
    ids = ref.encode_batch(texts)
    emb, proj = kc.probe_weights(256 + kc.PROBE_N_MERGES)
    worst = 0.0
    for fp8 in (False, True):
        st = kc.probe_score_stats(ids, emb, proj, fp8)
        assert st["min_lead"] >= 10 * kc.PROBE_SCORE_ALLOWANCE
        worst = max(worst, st["measured"])
    # the recorded figure is a measurement, not a guess: this machine's
    # fp32 evaluation may round differently, but must stay inside the
    # allowance derived from it
    assert 0.0 < worst <= kc.PROBE_SCORE_ALLOWANCE
    big = kc.probe_big_batch(texts)
    assert len(big) == 300 and sum(len(t) for t in big) > 66000
    assert min(len(t) for t in big) == 1 and big[170:] == texts
