"""CPU proof that check_topk_scoped (tests/kernel_checks.py) is sensitive:
it accepts the correct emulation of cache_topk_scoped on a planted masked
case and rejects eleven deliberately wrong emulations of plausible kernel
bugs, each with a message that names the broken property. The last tests
delete one structural feature of the case at a time and show that the
mutant it was there for then slips through, i.e. the case does the work."""

import pytest
import torch

import kernel_checks as kc

N_ROWS, DIM, NOW = 1103, 384, 1000  # 1024 + 64 + 15: ends in a 3-row group
DTYPES = [torch.bfloat16, torch.float8_e4m3fn]

# (winner, decoy) at the kernel's structural rows; every decoy shares its
# winner's 4-row lane group. 1102/1100: the winner sits in the final
# partial group whose first row is the ineligible decoy.
STRUCTURAL_PAIRS = [(1102, 1100), (15, 14), (255, 254), (1023, 1022), (0, 1),
                    (16, 17), (256, 257), (1024, 1025), (1088, 1089)]


def _proof_case(dtype, n_rows=N_ROWS, scope_bits=64, alias_passes=False):
    """256 queries (two 128-query passes). Query b's decoy kind is
    DECOY_KINDS[b % 4], so every fourth query is a wildcard and query b and
    b - 128 are of one kind. Unless alias_passes, the last two queries are
    one whose only eligible rows score below zero and one nothing may
    answer. The three keyword arguments each delete one feature:
    n_rows=1104 the partial group, scope_bits=31 the ids and decoy scopes
    that differ above bit 31 only, alias_passes the difference between
    q_scope[b] and q_scope[b - 128]."""
    n_normal = 256 if alias_passes else 254
    used = {r for p in STRUCTURAL_PAIRS for r in p} | set(range(1092, 1100))
    cands = [w for w in range(0, n_rows - 1, 2) if w not in used and w ^ 1 not in used]
    fill = [(w, w ^ 1) for w in cands[::2][: n_normal - len(STRUCTURAL_PAIRS)]]
    pairs = fill[:120] + STRUCTURAL_PAIRS + fill[120:]
    assert len(pairs) == n_normal
    scopes = kc.scope_ids(258, seed=77, bits=scope_bits)
    if alias_passes:
        scopes[128:256] = scopes[:128]
    queries = []
    for b, (w, d) in enumerate(pairs):
        k = b // 4 if scope_bits == 64 else 3  # 31-bit ids: successor scopes only
        queries.append(kc.scoped_query(w, scopes[b], d, kc.DECOY_KINDS[b % 4], NOW, k))
    if not alias_passes:
        k1, k0 = (1, 0) if scope_bits == 64 else (3, 3)
        queries.append(kc.ScopedQuery(1098, scopes[256], 1099,
                                      kc.foreign_scope(scopes[256], k1),
                                      negative=True, runner=1096))
        queries.append(kc.ScopedQuery(None, scopes[257], 1094,
                                      kc.foreign_scope(scopes[257], k0)))
    return kc.scoped_case(n_rows, DIM, dtype, queries, seed=202, now=NOW)


@pytest.fixture(scope="module", params=DTYPES, ids=["bf16", "fp8"])
def case(request):
    return _proof_case(request.param)


def _check(case, mutant=None):
    hi, idx = kc.emulate_topk_scoped(*case.tensors(), mutant=mutant)
    return kc.check_topk_scoped(hi, idx, *case.tensors(), shadowed=case.shadowed)


def test_scoped_correct_emulation_is_accepted(case):
    hi, idx = kc.emulate_topk_scoped(*case.tensors())
    stats = kc.check_topk_scoped(hi, idx, *case.tensors(), shadowed=case.shadowed)
    assert idx.tolist() == case.winners
    assert stats["min_gap"] > 0.4
    assert stats["min_shadow_lead"] > 0.05
    assert stats["max_err_over_bound"] <= 1.0
    # the case is what it says: both passes, ragged end, every decoy kind,
    # negative ids, a below-zero winner and an unanswerable query
    assert len(case.winners) == 256 and N_ROWS % 4 == 3
    assert len(case.shadowed) == 255 and case.winners[255] == -1
    qs = case.q_scope.tolist()
    assert qs.count(0) == 63 and sum(s < 0 for s in qs) > 64
    assert any(abs(s) >= 2 ** 32 for s in qs)
    assert int((case.row_expiry == NOW).sum()) >= 64


# mutant -> the property its rejection must name
SCOPED_MUTANTS = {
    "filter_after_argmax": "sentinel",
    "mask_after_group_max": "sentinel|wrong row",
    "expiry_ge": "ineligible row",
    "wildcard_ignores_expiry": "ineligible row",
    "second_pass_first_scopes": "wrong row|ineligible row|sentinel",
    "scope_low32": "ineligible row",
    "partial_group_ineligible": "wrong row|sentinel",
    "partial_group_first_tags": "wrong row|sentinel",
    "swapped_tile_tags": "wrong row|ineligible row|sentinel",
    "no_row_returns_row0": "sentinel",
    "nonpositive_lost": "sentinel",
}


def test_every_mutant_has_a_case():
    assert sorted(SCOPED_MUTANTS) == sorted(kc.SCOPED_MUTANTS)


@pytest.mark.parametrize("mutant", kc.SCOPED_MUTANTS)
def test_scoped_mutants_are_rejected(case, mutant):
    with pytest.raises(AssertionError, match=SCOPED_MUTANTS[mutant]) as exc:
        _check(case, mutant)
    assert "unfit" not in str(exc.value)


def test_scoped_mutants_fail_where_they_should(case):
    """The rejection comes from the query built for the mutant, not from a
    lucky side effect elsewhere: run each mutant and compare rows."""
    want = case.winners

    def wrong(mutant):
        _, idx = kc.emulate_topk_scoped(*case.tensors(), mutant=mutant)
        return {b for b, (g, w) in enumerate(zip(idx.tolist(), want)) if g != w}

    kinds = {k: {b for b in range(254) if b % 4 == i}
             for i, k in enumerate(kc.DECOY_KINDS)}
    assert wrong("expiry_ge") == kinds["now"]
    assert wrong("wildcard_ignores_expiry") == kinds["wild"]
    assert wrong("no_row_returns_row0") == {255}
    assert wrong("nonpositive_lost") == {254}
    assert wrong("partial_group_ineligible") == {120}  # the winner at row 1102
    assert wrong("partial_group_first_tags") == {120}
    assert wrong("second_pass_first_scopes") >= set(range(128, 256)) - kinds["wild"] - {255}
    assert wrong("second_pass_first_scopes") <= set(range(128, 256))
    # decoys whose scope differs above bit 31 only: foreign variants 0 and 1
    low32 = {b for b in kinds["foreign"] if (b // 4) % 4 in (0, 1)}
    assert wrong("scope_low32") == low32 | {254, 255}  # their decoys too
    assert wrong("filter_after_argmax") == set(range(255))
    assert wrong("mask_after_group_max") == set(range(255))
    # a wildcard query survives when the other tile's row happens to be alive
    assert wrong("swapped_tile_tags") >= set(range(254)) - kinds["wild"]


def test_scoped_score_bound_is_tight(case):
    """A right row with a score that is 1e-3 off must fail."""
    from aigw.ops.semcache import _unorder

    hi, idx = kc.emulate_topk_scoped(*case.tensors())
    for b in (5, 254):  # a positive and the negative maximum
        bad = list(hi)
        bad[b] = kc.order_float(_unorder(hi[b]) - 1e-3)
        with pytest.raises(AssertionError, match="bound"):
            kc.check_topk_scoped(bad, idx, *case.tensors(), shadowed=case.shadowed)


def test_scoped_sentinel_is_exact(case):
    """idx -1 with a non-zero hi, or a row with hi 0, is not the sentinel."""
    hi, idx = kc.emulate_topk_scoped(*case.tensors())
    bad = list(hi)
    bad[255] = kc.order_float(0.0)
    with pytest.raises(AssertionError, match="sentinel"):
        kc.check_topk_scoped(bad, idx, *case.tensors())
    bad_idx = idx.clone()
    bad_idx[255] = 1094  # the unanswerable query's decoy
    with pytest.raises(AssertionError, match="sentinel"):
        kc.check_topk_scoped(hi, bad_idx, *case.tensors())


def test_scoped_unfit_random_queries_are_refused():
    """Random unit queries with no planted winner: the masked gap of a
    wildcard query is ~0.008, no basis for an exact-row check."""
    index = kc.unit_rows(N_ROWS, DIM, torch.bfloat16, seed=5)
    q = kc.unit_rows(64, DIM, torch.bfloat16, seed=6)
    tags = (torch.ones(N_ROWS, dtype=torch.int64),
            torch.full((N_ROWS,), kc.NEVER, dtype=torch.int32),
            torch.zeros(64, dtype=torch.int64), NOW)
    hi, idx = kc.emulate_topk_scoped(index, q, *tags)
    with pytest.raises(AssertionError, match="unfit"):
        kc.check_topk_scoped(hi, idx, index, q, *tags)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp8"])
def test_scoped_unfit_shadow_flag_is_refused(dtype):
    """A query flagged as shadowed whose decoy is in fact eligible (same
    scope, alive): the decoy is then simply the winner, nothing out-scores
    it, and the flag is refused."""
    s = kc.scope_ids(2, seed=9)
    queries = [kc.scoped_query(40, s[0], 41, "foreign", NOW),
               kc.ScopedQuery(80, s[1], 82, decoy_scope=s[1], decoy_expiry=NOW + 1)]
    c = kc.scoped_case(N_ROWS, DIM, dtype, queries, seed=3, now=NOW)
    assert c.shadowed == [0]
    hi, idx = kc.emulate_topk_scoped(*c.tensors())
    assert idx.tolist() == [40, 82]
    kc.check_topk_scoped(hi, idx, *c.tensors(), shadowed=[0])
    with pytest.raises(AssertionError, match="unfit.*shadowed"):
        kc.check_topk_scoped(hi, idx, *c.tensors(), shadowed=[0, 1])


def test_scoped_case_refuses_two_roles_on_one_row():
    s = kc.scope_ids(2, seed=9)
    queries = [kc.scoped_query(40, s[0], 41, "foreign", NOW),
               kc.scoped_query(41, s[1], 42, "now", NOW)]
    with pytest.raises(AssertionError, match="collides"):
        kc.scoped_case(N_ROWS, DIM, torch.bfloat16, queries, seed=3, now=NOW)


def test_foreign_scopes_and_ids():
    ids = kc.scope_ids(500, seed=1)
    assert len(set(ids)) == 500 and 0 not in ids
    assert 150 < sum(i < 0 for i in ids) < 350
    for s in ids[:50] + [5, -5, 2 ** 62 + 3, -2 ** 62 - 3]:
        near = [kc.foreign_scope(s, k) for k in range(4)]
        assert len({s, *near}) == 5
        assert near[0] & 0xFFFFFFFF == s & 0xFFFFFFFF
        assert (near[1] < 0) != (s < 0) and near[1] & (2 ** 63 - 1) == s & (2 ** 63 - 1)
        assert all(-2 ** 63 <= v < 2 ** 63 for v in near)


# --- the case does the work: delete one feature, one mutant slips through ---

WEAKENED = [
    (dict(n_rows=1104), "partial_group_ineligible"),
    (dict(n_rows=1104), "partial_group_first_tags"),
    (dict(scope_bits=31), "scope_low32"),
    (dict(alias_passes=True), "second_pass_first_scopes"),
]


@pytest.mark.parametrize("weaken,mutant", WEAKENED,
                         ids=[f"{m}-{'-'.join(w)}" for w, m in WEAKENED])
def test_scoped_weakened_case_misses_its_mutant(weaken, mutant):
    weak = _proof_case(torch.bfloat16, **weaken)
    _check(weak)
    _check(weak, mutant)  # accepted: the deleted feature was what caught it
    with pytest.raises(AssertionError):
        _check(_proof_case(torch.bfloat16), mutant)
