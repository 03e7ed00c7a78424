"""cache_topk_scoped edge tests: the scope- and TTL-filtered lookup held to
exact rows under the mask. Planted masked inputs (kernel_checks.scoped_case):
every query has one eligible winner (~0.9) and, where the test says so, an
ineligible decoy that strictly out-scores it (an exact copy of the query).
check_topk_scoped compares with the masked fp64 product under the a-priori
fp32 bound and refuses inputs whose gaps do not clear 100x that bound;
tests/test_kernel_checks_scoped_cpu.py proves it rejects eleven wrong
emulations of the kernel."""

import pytest
import torch

import kernel_checks as kc
from kernel_checks import INT32_MIN, NEVER

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float8_e4m3fn]
DTYPE_IDS = ["bf16", "fp8"]
N_ROWS = 1103  # 1024 + 64 + 15: a partial last tile that ends in a 3-row group
NOW = 1000


@pytest.fixture(scope="module")
def hip():
    import aigw_hip

    return aigw_hip


def _run(hip, index, q, row_scope, row_expiry, q_scope, now):
    hi, idx = hip.cache_topk_scoped(index.cuda(), q.cuda(), row_scope.cuda(),
                                    row_expiry.cuda(), q_scope.cuda(), now)
    return hi.cpu(), idx.cpu()


def _run_case(hip, c, winners=None):
    """Runs the kernel on a ScopedCase: checked against the masked fp64
    reference, and the rows must be exactly the planted winners."""
    hi, idx = _run(hip, *c.tensors())
    stats = kc.check_topk_scoped(hi, idx, *c.tensors(), shadowed=c.shadowed)
    assert idx.tolist() == (c.winners if winners is None else winners)
    return stats


def _same_group_decoy(w, n_rows):
    return w ^ 1 if w ^ 1 < n_rows else w - 1


# ---------------------------------------------------------------------------
# 1. every row wins once under the mask
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_every_row_wins_once_under_the_mask(hip, dtype):
    """dim 384, 1103 rows: over six calls every row is the exact masked
    argmax of exactly one query while its pair partner w ^ 1 (same lane
    group; above an even winner, below an odd one) holds an ineligible copy
    of the query. Decoy kinds cycle: foreign scope, expiry == now,
    expiry < now, wildcard query with an expired decoy."""
    worst, min_gap, min_lead, seen = 0.0, float("inf"), float("inf"), []
    call = 0
    for parity in (0, 1):
        rows = list(range(parity, N_ROWS, 2))
        for lo in range(0, len(rows), 256):
            winners = rows[lo:lo + 256]
            scopes = kc.scope_ids(len(winners), seed=900 + call)
            queries = kc.pair_queries(winners, scopes, N_ROWS, NOW, start=call)
            c = kc.scoped_case(N_ROWS, 384, dtype, queries, seed=384 + call, now=NOW)
            # every winner whose partner exists is shadowed by it
            assert len(c.shadowed) == sum(w ^ 1 < N_ROWS for w in winners)
            stats = _run_case(hip, c, winners)
            worst = max(worst, stats["max_err_over_bound"])
            min_gap = min(min_gap, stats["min_gap"])
            min_lead = min(min_lead, stats["min_shadow_lead"])
            seen += winners
            call += 1
    assert sorted(seen) == list(range(N_ROWS)) and call == 6
    print(f"scoped sweep {dtype}: max |err|/bound = {worst:.3f}, "
          f"min gap {min_gap:.3f}, min shadow lead {min_lead:.3f}")
    assert min_gap > 0.4 and min_lead > 0.05


# ---------------------------------------------------------------------------
# 2. decoy placements
# ---------------------------------------------------------------------------

# (winner, decoy); the second call swaps every pair, so each placement is
# run with the decoy below and above the winner
PLACEMENTS = [
    (38, 37), (41, 43),          # same 4-row lane group, decoy lower / higher
    (50, 60), (77, 66),          # same 16-row tile, another group
    (15, 16),                    # across a tile edge
    (255, 256),                  # across the 256-row wave span
    (1023, 1024),                # across the 1024-row block edge
    (1100, 1102),                # inside the final partial group
    (1040, 100), (200, 1060),    # block 1 winner / block 0 decoy and the reverse
    (300, 20), (700, 1101),      # another wave; decoy in the partial group
]


@pytest.mark.parametrize("swap", [False, True], ids=["as_listed", "swapped"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_decoy_placements(hip, dtype, swap):
    pairs = [(d, w) if swap else (w, d) for w, d in PLACEMENTS]
    scopes = kc.scope_ids(len(pairs), seed=31)
    queries = [kc.scoped_query(w, s, d, kc.DECOY_KINDS[i % 4], NOW, i // 4)
               for i, ((w, d), s) in enumerate(zip(pairs, scopes))]
    c = kc.scoped_case(N_ROWS, 384, dtype, queries, seed=32, now=NOW)
    assert len(c.shadowed) == len(pairs)
    stats = _run_case(hip, c)
    assert stats["min_shadow_lead"] > 0.05


# ---------------------------------------------------------------------------
# 3. all four dims
# ---------------------------------------------------------------------------

STRUCTURAL = [0, 15, 16, 255, 256, 1023, 1024, 1088, 1102]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("dim", [128, 256, 384, 512])
def test_structural_winners_all_dims(hip, dim, dtype):
    """The dim-256 and dim-512 instantiations run here for the first time."""
    scopes = kc.scope_ids(len(STRUCTURAL) + 2, seed=dim)
    queries = [kc.scoped_query(w, s, _same_group_decoy(w, N_ROWS),
                               ("foreign", "now", "past")[i % 3], NOW, i)
               for i, (w, s) in enumerate(zip(STRUCTURAL, scopes))]
    queries.append(kc.scoped_query(600, scopes[-2], 601, "wild", NOW))
    queries.append(kc.ScopedQuery(None, scopes[-1], 700, kc.foreign_scope(scopes[-1], 1)))
    c = kc.scoped_case(N_ROWS, dim, dtype, queries, seed=dim + 1, now=NOW)
    assert c.q_scope.tolist().count(0) == 1
    stats = _run_case(hip, c, STRUCTURAL + [600, -1])
    print(f"scoped dim {dim} {dtype}: {stats}")


# ---------------------------------------------------------------------------
# 4. query-count edges
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n_q", [1, 16, 17, 127, 128, 129, 255, 256])
def test_query_count_edges(hip, n_q, dtype):
    """Every query has its own scope and winner. Query b's decoy (same lane
    group) carries the scope of query b +- 128 where that query exists, so
    a 128-query pass that reads the other pass's q_scope slice returns the
    decoy."""
    scopes = kc.scope_ids(n_q, seed=40 + n_q)
    queries = []
    for b in range(n_q):
        other = b - 128 if b >= 128 else b + 128
        ds = scopes[other] if other < n_q else kc.foreign_scope(scopes[b], b)
        queries.append(kc.ScopedQuery(4 * b + b % 3, scopes[b], 4 * b + 3, ds))
    c = kc.scoped_case(N_ROWS, 384, dtype, queries, seed=41, now=NOW)
    assert len(c.shadowed) == n_q
    _run_case(hip, c)


# ---------------------------------------------------------------------------
# 5. row-count edges with poisoned slack
# ---------------------------------------------------------------------------

ROW_COUNTS = [1, 2, 3, 4, 5, 6, 7, 13, 15, 16, 17, 18, 19, 255, 256, 257, 258,
              1023, 1024, 1025, 1026, 1027]
SLACK = 64


def _with_poisoned_slack(c):
    """[:n_rows] views (from row 0, so aligned) of GPU allocations 64 rows
    longer whose slack rows are exact copies of query 0 with its scope and
    expiry NEVER: reading a row or a tag past n_rows changes the answer."""
    n = c.index.shape[0]
    index = torch.cat([c.index, c.q[:1].expand(SLACK, -1)]).cuda()
    rs = torch.cat([c.row_scope, c.q_scope[:1].expand(SLACK)]).cuda()
    re = torch.cat([c.row_expiry,
                    torch.full((SLACK,), NEVER, dtype=torch.int32)]).cuda()
    assert rs.data_ptr() % 32 == 0 and re.data_ptr() % 16 == 0
    return index[:n], c.q.cuda(), rs[:n], re[:n], c.q_scope.cuda(), c.now


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_row_count_edges_with_poisoned_slack(hip, dtype):
    """One scoped query per call. The winner is the last row with its decoy
    at n_rows - 2, then the other way round; then every row below n_rows is
    made ineligible so that only the slack could answer. Nothing here reads
    out of bounds on purpose: an accidental over-read shows as a wrong row."""
    for i, n_rows in enumerate(ROW_COUNTS):
        scope = kc.scope_ids(1, seed=5000 + n_rows)[0]
        kind = ("foreign", "now", "past")[i % 3]
        layouts = [(n_rows - 1, n_rows - 2 if n_rows >= 2 else None)]
        if n_rows >= 2:
            layouts.append((n_rows - 2, n_rows - 1))
        for w, d in layouts:
            c = kc.scoped_case(n_rows, 384, dtype,
                               [kc.scoped_query(w, scope, d, kind, NOW, i)],
                               seed=5100 + n_rows, now=NOW)
            hi, idx = hip.cache_topk_scoped(*_with_poisoned_slack(c))
            hi, idx = hi.cpu(), idx.cpu()
            assert int(idx[0]) < n_rows, (n_rows, w, d, idx.tolist())
            kc.check_topk_scoped(hi, idx, *c.tensors(), shadowed=c.shadowed)
            assert idx.tolist() == [w], (n_rows, w, d)
        # nothing below n_rows may answer: odd rows dead, even rows foreign
        c.row_expiry[1::2] = (NOW, NOW - 1)[i % 2]
        c.row_scope[0::2] = kc.foreign_scope(scope, i)
        hi, idx = hip.cache_topk_scoped(*_with_poisoned_slack(c))
        assert idx.cpu().tolist() == [-1] and hi.cpu().tolist() == [0], n_rows
        kc.check_topk_scoped(hi, idx, *c.tensors())


# ---------------------------------------------------------------------------
# 6. the best == 0 sentinel against real scores
# ---------------------------------------------------------------------------

NEG_WINNER, NEG_DEAD, NEG_FOREIGN = 301, 300, 303
ZERO_FIRST = 600


def _sentinel_case(dtype):
    """Rows 0..599, scope A: every row anti-correlated with the A queries,
    as in test_topk_all_negative_scores. Row 301 (c = 0.3, about -0.29) is
    the least negative eligible one; row 300 (c = 0.05) is less negative but
    expired at `now`, row 303 (c = 0.1) less negative under a foreign scope.
    Rows 600..1102, scope B: zero vectors, except copies of the B query at
    601 (foreign scope) and 1101 (expired). Scope C matches nothing."""
    g = torch.Generator().manual_seed(61)
    dim = 384
    sa, sb, sc = kc.scope_ids(3, seed=62)
    u = torch.nn.functional.normalize(torch.randn(dim, generator=g), dim=0)
    w = torch.nn.functional.normalize(torch.randn(ZERO_FIRST, dim, generator=g), dim=1)
    cw = 1.0 + 2.0 * torch.rand(ZERO_FIRST, generator=g)
    cw[NEG_WINNER], cw[NEG_DEAD], cw[NEG_FOREIGN] = 0.3, 0.05, 0.1
    index = torch.zeros(N_ROWS, dim)
    index[:ZERO_FIRST] = -torch.nn.functional.normalize(cw[:, None] * u + w, dim=1)
    noise = torch.randn(6, dim, generator=g) / dim ** 0.5
    qa = torch.nn.functional.normalize(u + 0.1 * noise, dim=1)
    qb = torch.nn.functional.normalize(torch.randn(dim, generator=g), dim=0)
    qb = qb.to(torch.bfloat16).to(dtype).float()
    index[601] = qb
    index[1101] = qb
    row_scope = torch.tensor([sa] * ZERO_FIRST + [sb] * (N_ROWS - ZERO_FIRST))
    row_expiry = torch.full((N_ROWS,), NEVER, dtype=torch.int32)
    row_expiry[NEG_DEAD] = NOW
    row_scope[NEG_FOREIGN] = kc.foreign_scope(sa, 1)
    row_scope[601] = kc.foreign_scope(sb, 0)
    row_expiry[1101] = NOW - 1
    index = index.to(torch.bfloat16).to(dtype)
    qa = qa.to(torch.bfloat16).to(dtype)
    qb = qb.to(torch.bfloat16).to(dtype)
    zero_rows = set(range(ZERO_FIRST, N_ROWS)) - {601, 1101}
    return index, qa, qb, row_scope, row_expiry, (sa, sb, sc), zero_rows


def _sentinel_run(hip, dtype, kinds):
    """kinds: one of "neg", "zero", "none" per query."""
    from aigw.ops.semcache import _unorder

    index, qa, qb, rs, re, (sa, sb, sc), zero_rows = _sentinel_case(dtype)
    rows, scopes, allowed = [], [], []
    for i, kind in enumerate(kinds):
        rows.append(qa[i % qa.shape[0]] if kind == "neg" else qb)
        scopes.append({"neg": sa, "zero": sb, "none": sc}[kind])
        allowed.append(zero_rows if kind == "zero" else None)
    q = torch.stack(rows)
    qs = torch.tensor(scopes, dtype=torch.int64)
    hi, idx = _run(hip, index, q, rs, re, qs, NOW)
    shadowed = [i for i, k in enumerate(kinds) if k != "none"]
    stats = kc.check_topk_scoped(hi, idx, index, q, rs, re, qs, NOW,
                                 allowed_rows=allowed, shadowed=shadowed)
    for i, kind in enumerate(kinds):
        if kind == "neg":
            assert int(idx[i]) == NEG_WINNER and _unorder(int(hi[i])) < -0.2, (i, idx)
        elif kind == "zero":
            assert int(idx[i]) in zero_rows and _unorder(int(hi[i])) == 0.0, (i, idx)
        else:
            assert int(idx[i]) == -1 and int(hi[i]) == 0, (i, idx)
    return stats


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_all_negative_eligible_scores(hip, dtype):
    """best_s starts at 0.f and the orderable-float transform takes its
    negative branch: the least negative eligible row comes back, not -1 and
    not one of the two less negative ineligible rows."""
    stats = _sentinel_run(hip, dtype, ["neg"] * 6)
    assert stats["min_gap"] > 0.1 and stats["min_shadow_lead"] > 0.04


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_eligible_rows_scoring_exactly_zero(hip, dtype):
    """Every eligible row is a zero vector while an ineligible row scores
    |q|^2: a zero row comes back with score exactly 0.0, not the sentinel."""
    stats = _sentinel_run(hip, dtype, ["zero"] * 3)
    assert stats["min_shadow_lead"] > 0.5


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_sentinel_mixed_batch(hip, dtype):
    _sentinel_run(hip, dtype, ["none", "neg", "zero"] * 6 + ["none"])


# ---------------------------------------------------------------------------
# 7. clock and tag extremes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("now", [0, -5, NEVER - 1])
def test_clock_and_expiry_extremes(hip, now, dtype):
    """Per expiry extreme one scoped and one wildcard query: a copy of the
    query with that expiry (and the query's scope) next to a planted winner
    that never expires. The copy wins iff its expiry > now."""
    expiries = [INT32_MIN, 0, now, now + 1, NEVER]
    scopes = kc.scope_ids(len(expiries), seed=70)
    queries, want = [], []
    for i, e in enumerate(expiries):
        for wild in (False, True):
            w, d = 12 * len(queries) + 2, 12 * len(queries) + 3
            queries.append(kc.ScopedQuery(w, 0 if wild else scopes[i], d, scopes[i],
                                          decoy_expiry=e, winner_expiry=NEVER))
            want.append(d if e > now else w)
    c = kc.scoped_case(131, 128, dtype, queries, seed=71, now=now)
    assert len(c.shadowed) == sum(r == q.winner for r, q in zip(want, queries))
    assert 0 < len(c.shadowed) < len(queries)
    _run_case(hip, c, want)


def test_now_out_of_int32_range_raises(hip):
    c = kc.scoped_case(16, 128, torch.bfloat16,
                       [kc.ScopedQuery(3, 5)], seed=72, now=NOW)
    index, q, rs, re, qs, _ = (t.cuda() if isinstance(t, torch.Tensor) else t
                               for t in c.tensors())
    hip.cache_topk_scoped(index, q, rs, re, qs, 2 ** 31 - 1)
    hip.cache_topk_scoped(index, q, rs, re, qs, -2 ** 31)
    for bad in (2 ** 31, -2 ** 31 - 1):
        with pytest.raises(RuntimeError):
            hip.cache_topk_scoped(index, q, rs, re, qs, bad)


# ---------------------------------------------------------------------------
# 8. wrapper contract
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def offset_case():
    """A structural case behind four poison rows: exact copies of query 0
    under its scope, alive. A lookup over the [4:] views must not see them."""
    scopes = kc.scope_ids(len(STRUCTURAL), seed=80)
    queries = [kc.scoped_query(w, s, _same_group_decoy(w, N_ROWS),
                               kc.DECOY_KINDS[i % 4], NOW, i)
               for i, (w, s) in enumerate(zip(STRUCTURAL, scopes))]
    assert queries[0].scope != 0
    c = kc.scoped_case(N_ROWS, 384, torch.bfloat16, queries, seed=81, now=NOW)
    index = torch.cat([c.q[:1].expand(4, -1), c.index]).cuda()
    rs = torch.cat([c.q_scope[:1].expand(4), c.row_scope]).cuda()
    re = torch.cat([torch.full((4,), NEVER, dtype=torch.int32), c.row_expiry]).cuda()
    assert rs.data_ptr() % 32 == 0 and re.data_ptr() % 16 == 0
    return c, index, rs, re


def test_views_from_row_4_are_served(hip, offset_case):
    c, index, rs, re = offset_case
    q, qs = c.q.cuda(), c.q_scope.cuda()
    hi, idx = hip.cache_topk_scoped(index[4:], q, rs[4:], re[4:], qs, NOW)
    kc.check_topk_scoped(hi, idx, *c.tensors(), shadowed=c.shadowed)
    assert idx.cpu().tolist() == STRUCTURAL  # numbered relative to the view
    # over the whole allocation query 0 finds a poison row instead
    _, idx = hip.cache_topk_scoped(index, q, rs, re, qs, NOW)
    assert 0 <= int(idx[0]) < 4


def test_misaligned_tag_views_are_refused(hip, offset_case):
    c, index, rs, re = offset_case
    q, qs = c.q.cuda(), c.q_scope.cuda()
    rs_ok, re_ok = rs[1:].clone(), re[1:].clone()
    assert rs_ok.data_ptr() % 32 == 0 and re_ok.data_ptr() % 16 == 0
    hip.cache_topk_scoped(index[1:], q, rs_ok, re_ok, qs, NOW)
    for bad_rs, bad_re in [(rs[1:], re[1:]), (rs[1:], re_ok), (rs_ok, re[1:])]:
        with pytest.raises(RuntimeError):
            hip.cache_topk_scoped(index[1:], q, bad_rs, bad_re, qs, NOW)


def test_empty_and_oversized_calls(hip, offset_case):
    c, index, rs, re = offset_case
    q, qs = c.q.cuda(), c.q_scope.cuda()
    hi, idx = hip.cache_topk_scoped(index, q[:0], rs, re, qs[:0], NOW)
    assert hi.shape == (0,) and idx.shape == (0,)
    assert hi.dtype == torch.int64 and idx.dtype == torch.int32
    hi, idx = hip.cache_topk_scoped(index[:0], q, rs[:0], re[:0], qs, NOW)
    assert idx.cpu().tolist() == [-1] * len(STRUCTURAL)
    assert hi.cpu().tolist() == [0] * len(STRUCTURAL)
    q257 = q[:1].expand(257, -1).contiguous()
    qs257 = qs[:1].expand(257).contiguous()
    with pytest.raises(RuntimeError):
        hip.cache_topk_scoped(index, q257, rs, re, qs257, NOW)
    hip.cache_topk_scoped(index, q257[:256], rs, re, qs257[:256], NOW)
