"""Comparators and input builders for the HIP kernel edge tests.

Plain helper module (no tests here): tests/test_kernel_checks_cpu.py and
tests/test_kernel_checks_scoped_cpu.py prove on the CPU that each comparator
rejects deliberately wrong emulations, and tests/test_gpu_kernel_edges.py
and tests/test_gpu_cache_scoped_edges.py feed them the real kernels' outputs.

Every bound below is an a-priori floating-point error bound for the
operation, never a figure taken from the kernel under test.
"""

from __future__ import annotations

import struct

import numpy as np
import torch

EPS23 = 2.0 ** -23  # twice the fp32 unit roundoff


# ---------------------------------------------------------------------------
# cache_topk
# ---------------------------------------------------------------------------

def order_float(s: float) -> int:
    """pack_score's orderable-float transform (inverse of semcache._unorder)."""
    u = struct.unpack("<I", struct.pack("<f", float(s)))[0]
    return (~u & 0xFFFFFFFF) if (u & 0x80000000) else (u | 0x80000000)


def _as_list(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().tolist()
    return list(x)


def check_topk(hi, idx, index, q, allowed_rows=None) -> dict:
    """Exact-row check of a cache_topk result against the fp64 product.

    `index` (N, dim) and `q` (B, dim) are the already quantised (bf16 or
    e4m3) operands, so their fp64 product is the exact score matrix. For
    each query the returned row must be the fp64 argmax (or, for a
    deliberate exact tie, any member of allowed_rows[b]) and the returned
    score must lie within the fp32 dot-product bound
    dim * 2^-23 * |index[row]| * |q[b]| of the exact maximum (dim * 2^-24
    is the classic bound for any summation order; 2x margin).

    The inputs themselves are checked too: the exact top-1/top-2 gap must
    exceed 100x that bound, otherwise an exact-row assertion would be a
    coin toss. Returns the worst figures seen, for reporting.
    """
    # the unfiltered lookup is the scoped one with every cell eligible
    n_rows, n_q = index.shape[0], q.shape[0]
    stats = check_topk_scoped(
        hi, idx, index, q, torch.zeros(n_rows, dtype=torch.int64),
        torch.full((n_rows,), NEVER, dtype=torch.int32),
        torch.zeros(n_q, dtype=torch.int64), 0, allowed_rows)
    del stats["min_shadow_lead"]
    return stats


def unit_rows(n_rows: int, dim: int, dtype, seed: int) -> torch.Tensor:
    """Seeded random unit rows, quantised to `dtype` (CPU tensor)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.normalize(
        torch.randn(n_rows, dim, generator=g), dim=1)
    return x.to(torch.bfloat16).to(dtype)


def planted_case(n_rows: int, dim: int, dtype, winners, seed: int):
    """Planted-winner inputs: random unit background, query b IS index row
    winners[b], so that row scores ~1 against ~0.2 for the best other row."""
    index = unit_rows(n_rows, dim, dtype, seed)
    q = index[torch.as_tensor(list(winners), dtype=torch.long)].clone()
    return index, q


def emulate_topk(index, q, row_mask=None, alias_second_pass=False):
    """Pure-torch fp32 emulation of cache_topk's contract -> (hi, idx).

    row_mask (bool per index row) and alias_second_pass exist only so the
    CPU self-tests can build deliberately wrong variants."""
    s = index.to(torch.float32) @ q.to(torch.float32).T  # (N, B)
    if row_mask is not None:
        s = s.masked_fill(~row_mask[:, None], -1e30)
    val, idx = s.max(dim=0)
    idx = idx.clone()
    if alias_second_pass:
        idx[128:] = idx[: max(idx.numel() - 128, 0)]
    hi = [order_float(v) for v in val.tolist()]
    return hi, idx.to(torch.int32)


# ---------------------------------------------------------------------------
# cache_topk_scoped
# ---------------------------------------------------------------------------

NEVER = 0x7FFFFFFF  # row_expiry of a row without a TTL
INT32_MIN = -2 ** 31
_INT64_MIN, _INT64_MAX = -2 ** 63, 2 ** 63 - 1


def _i64_cpu(x) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().to(torch.int64)
    return torch.tensor(list(x), dtype=torch.int64)


def scoped_eligibility(row_scope, row_expiry, q_scope, now) -> torch.Tensor:
    """(n_rows, n_q) bool on the CPU: row r may answer query j iff
    row_expiry[r] > now and (q_scope[j] == 0 or row_scope[r] == q_scope[j])."""
    rs, re, qs = _i64_cpu(row_scope), _i64_cpu(row_expiry), _i64_cpu(q_scope)
    live = (re > int(now))[:, None]
    match = (qs == 0)[None, :] | (rs[:, None] == qs[None, :])
    return live & match


def check_topk_scoped(hi, idx, index, q, row_scope, row_expiry, q_scope, now,
                      allowed_rows=None, shadowed=()) -> dict:
    """check_topk under the scope/TTL mask.

    The reference is the fp64 product of the quantised operands with every
    ineligible cell (scoped_eligibility) at -inf. A query nothing may
    answer must come back as exactly idx -1 / hi 0. Any other query must
    get the exact masked argmax (or a member of allowed_rows[b]), that row
    must be eligible, and the score must lie within check_topk's bound,
    dim * 2^-23 * |row| * |q|, of the exact masked maximum.

    Input fitness: the masked top-1/top-2 gap must exceed 100x the bound,
    and for every query listed in `shadowed` the unmasked maximum must
    exceed the masked one by more than 100x the bound, i.e. an ineligible
    row really does out-score the winner. Each assertion names the failed
    property: "sentinel", "ineligible row", "wrong row" or "bound"."""
    from aigw.ops.semcache import _unorder

    hi = _as_list(hi)
    idx = _as_list(idx)
    index64 = index.detach().cpu().to(torch.float64)
    q64 = q.detach().cpu().to(torch.float64)
    n_rows, dim = index64.shape
    n_q = q64.shape[0]
    assert len(hi) == n_q and len(idx) == n_q, (len(hi), len(idx), n_q)
    elig = scoped_eligibility(row_scope, row_expiry, q_scope, now)
    assert tuple(elig.shape) == (n_rows, n_q), tuple(elig.shape)
    S = index64 @ q64.T
    row_norm = index64.norm(dim=1)
    q_norm = q64.norm(dim=1)
    max_row_norm = float(row_norm.max()) if n_rows else 0.0
    shadowed = {int(b) for b in shadowed}
    worst_err, worst_ratio = 0.0, 0.0
    min_gap, min_lead = float("inf"), float("inf")
    for b in range(n_q):
        col, ok = S[:, b], elig[:, b]
        row = int(idx[b])
        if not bool(ok.any()):
            assert b not in shadowed, (
                f"query {b}: inputs unfit, flagged shadowed but no row is eligible")
            assert row == -1 and int(hi[b]) == 0, (
                f"query {b}: sentinel: no row is eligible, want idx -1 / hi 0, "
                f"got idx {row} / hi {int(hi[b])}")
            continue
        masked = col.masked_fill(~ok, -float("inf"))
        smax = float(masked.max())
        if allowed_rows is not None and allowed_rows[b] is not None:
            allowed = sorted(int(r) for r in allowed_rows[b])
            for r in allowed:
                assert float(masked[r]) == smax, (
                    f"query {b}: allowed row {r} scores {float(masked[r])!r} under "
                    f"the mask, not the exact maximum {smax!r}")
        else:
            allowed = [int(masked.argmax())]
        gap_tol = dim * EPS23 * max_row_norm * float(q_norm[b])
        rest = masked.clone()
        rest[allowed] = -float("inf")
        second = float(rest.max())
        if second > -float("inf"):
            gap = smax - second
            assert gap > 100.0 * gap_tol, (
                f"query {b}: inputs unfit for an exact-row check, masked "
                f"top-1/top-2 gap {gap:.3e} <= 100 x {gap_tol:.3e}")
            min_gap = min(min_gap, gap)
        if b in shadowed:
            lead = float(col.max()) - smax
            assert lead > 100.0 * gap_tol, (
                f"query {b}: inputs unfit, flagged shadowed but the best ineligible "
                f"row leads the masked maximum by {lead:.3e} <= 100 x {gap_tol:.3e}")
            min_lead = min(min_lead, lead)
        assert row != -1, (
            f"query {b}: sentinel: got idx -1 / hi {int(hi[b])} although row "
            f"{allowed[0]} is eligible (exact score {smax:.6f})")
        assert 0 <= row < n_rows, f"query {b}: row {row} out of range"
        assert bool(ok[row]), (
            f"query {b}: ineligible row {row} (scope {int(_i64_cpu(row_scope)[row])}, "
            f"expiry {int(_i64_cpu(row_expiry)[row])}) returned for scope "
            f"{int(_i64_cpu(q_scope)[b])} at now {int(now)}; want one of {allowed[:8]}")
        assert row in allowed, (
            f"query {b}: wrong row: got row {row} (exact score {float(col[row]):.6f}), "
            f"want one of {allowed[:8]} (exact score {smax:.6f})")
        score = _unorder(int(hi[b]))
        tol = dim * EPS23 * float(row_norm[row]) * float(q_norm[b])
        err = abs(score - smax)
        assert err <= tol, (
            f"query {b}: score {score!r} vs exact {smax!r}: "
            f"|err| {err:.3e} > bound {tol:.3e}")
        worst_err = max(worst_err, err)
        if tol > 0:
            worst_ratio = max(worst_ratio, err / tol)
    return {"max_err": worst_err, "max_err_over_bound": worst_ratio,
            "min_gap": min_gap, "min_shadow_lead": min_lead}


SCOPED_MUTANTS = (
    "filter_after_argmax",        # a
    "mask_after_group_max",       # b
    "expiry_ge",                  # c
    "wildcard_ignores_expiry",    # d
    "second_pass_first_scopes",   # e
    "scope_low32",                # f
    "partial_group_ineligible",   # g
    "partial_group_first_tags",   # h
    "swapped_tile_tags",          # i
    "no_row_returns_row0",        # j
    "nonpositive_lost",           # k
)


def emulate_topk_scoped(index, q, row_scope, row_expiry, q_scope, now, mutant=None):
    """Pure-torch fp32 emulation of cache_topk_scoped's contract -> (hi, idx).

    `mutant` (one of SCOPED_MUTANTS) exists only so the CPU self-tests can
    build deliberately wrong variants of the kernel's structure: 4-row lane
    groups, 16-row tiles with ping-pong tag buffers, 128-query passes."""
    assert mutant is None or mutant in SCOPED_MUTANTS, mutant
    s = index.to(torch.float32) @ q.to(torch.float32).T  # (N, B)
    n_rows, n_q = s.shape
    rs, re, qs = _i64_cpu(row_scope), _i64_cpu(row_expiry), _i64_cpu(q_scope)
    in_range = torch.ones(n_rows, dtype=torch.bool)
    rows = torch.arange(n_rows)
    tail0 = (n_rows // 4) * 4  # first row of the partial 4-row group, if any
    if mutant == "partial_group_ineligible":
        in_range = rows < tail0
    if mutant == "partial_group_first_tags" and tail0 < n_rows:
        rs, re = rs.clone(), re.clone()
        rs[tail0:] = rs[tail0]
        re[tail0:] = re[tail0]
    if mutant == "swapped_tile_tags":
        src = rows ^ 16
        in_range = src < n_rows
        src = src.clamp_max(n_rows - 1)
        rs, re = rs[src], re[src]
    if mutant == "second_pass_first_scopes":
        qs = qs.clone()
        qs[128:] = qs[: max(n_q - 128, 0)]
    live = (re >= now) if mutant == "expiry_ge" else (re > now)
    wild = (qs == 0)[None, :]
    if mutant == "scope_low32":
        match = wild | ((rs & 0xFFFFFFFF)[:, None] == (qs & 0xFFFFFFFF)[None, :])
    else:
        match = wild | (rs[:, None] == qs[None, :])
    elig = live[:, None] & match
    if mutant == "wildcard_ignores_expiry":
        elig = elig | wild.expand(n_rows, n_q)
    elig = elig & in_range[:, None]
    if mutant == "nonpositive_lost":
        elig = elig & (s > 0)
    neg = torch.full_like(s, -float("inf"))
    cols = torch.arange(n_q)
    if mutant == "filter_after_argmax":
        val, idx = s.max(dim=0)
        found = elig[idx, cols]
    elif mutant == "mask_after_group_max":
        pad = (-n_rows) % 4
        sp = torch.cat([s, neg[:pad]])
        ep = torch.cat([elig, torch.zeros(pad, n_q, dtype=torch.bool)])
        gval, gr = sp.view(-1, 4, n_q).max(dim=1)  # unfiltered best of each group
        grow = gr + 4 * torch.arange(sp.shape[0] // 4)[:, None]
        gok = ep[grow, cols[None, :]]
        val, g = torch.where(gok, gval, neg[: gval.shape[0]]).max(dim=0)
        idx = grow[g, cols]
        found = gok.any(dim=0)
    else:
        val, idx = torch.where(elig, s, neg).max(dim=0)
        found = elig.any(dim=0)
    hi, out = [], []
    for b in range(n_q):
        if bool(found[b]):
            hi.append(order_float(float(val[b])))
            out.append(int(idx[b]))
        elif mutant == "no_row_returns_row0":
            hi.append(order_float(float(s[0, b])))
            out.append(0)
        else:
            hi.append(0)
            out.append(-1)
    return hi, torch.tensor(out, dtype=torch.int32)


def scope_ids(n: int, seed: int, bits: int = 64) -> list[int]:
    """n distinct seeded scope ids over the full signed int64 range (as the
    first 8 bytes of a SHA-256 are), about half of them negative; never 0
    (the wildcard), and never a value whose foreign_scope() would overflow
    or hit 0. bits=31 gives small positive ids instead (only for the
    self-tests that show what 64-bit ids add)."""
    rng = np.random.default_rng(seed)
    out, seen = [], {0, -1, 1, _INT64_MIN, _INT64_MAX}
    while len(out) < n:
        if bits == 64:
            v = int(rng.integers(_INT64_MIN, _INT64_MAX, dtype=np.int64, endpoint=True))
        else:
            v = int(rng.integers(2, 2 ** bits - 2))
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def foreign_scope(s: int, k: int) -> int:
    """A scope id that is not `s` but is close to it in one of four ways:
    the low 32 bits equal, all but the sign bit equal, the negation, the
    successor."""
    k %= 4
    if k == 0:
        v = s ^ (1 << 32)
    elif k == 1:
        v = s + 2 ** 63 if s < 0 else s - 2 ** 63  # s ^ (1 << 63) as signed
    elif k == 2:
        v = -s
    else:
        v = s + 1
    assert v != s and v != 0 and _INT64_MIN <= v <= _INT64_MAX, (s, k, v)
    return v


class ScopedQuery:
    """One query of a planted masked case.

    winner      row that must come back, or None for a query nothing may
                answer (its scope then matches no row)
    scope       the query's scope id, 0 = wildcard
    decoy       row that gets an exact copy of the query, or None
    decoy_scope, decoy_expiry   the decoy's tag (decoy_scope None = `scope`)
    winner_expiry               the winner's expiry (None = builder's choice)
    negative    the winner is -0.5 * query and `runner` is -query, the only
                two rows of the query's scope: the masked maximum is < 0
    """

    def __init__(self, winner, scope, decoy=None, decoy_scope=None,
                 decoy_expiry=NEVER, winner_expiry=None, negative=False, runner=None):
        self.winner, self.scope, self.decoy = winner, int(scope), decoy
        self.decoy_scope = self.scope if decoy_scope is None else int(decoy_scope)
        self.decoy_expiry, self.winner_expiry = int(decoy_expiry), winner_expiry
        self.negative, self.runner = negative, runner
        assert (runner is not None) == negative


DECOY_KINDS = ("foreign", "now", "past", "wild")


def scoped_query(winner, scope, decoy, kind, now, k=0) -> ScopedQuery:
    """A ScopedQuery whose decoy is ineligible in the way `kind` says:
    foreign scope (variant k of foreign_scope), expiry == now, expiry < now,
    or a wildcard query with an expired decoy."""
    if decoy is None:
        return ScopedQuery(winner, scope)
    if kind == "foreign":
        return ScopedQuery(winner, scope, decoy, foreign_scope(scope, k))
    if kind == "now":
        return ScopedQuery(winner, scope, decoy, decoy_expiry=now)
    if kind == "past":
        return ScopedQuery(winner, scope, decoy,
                           decoy_expiry=(now - 1, 0, INT32_MIN)[k % 3] if now > 0 else now - 1)
    assert kind == "wild", kind
    return ScopedQuery(winner, 0, decoy, decoy_scope=scope, decoy_expiry=now - 1 - k % 2)


class ScopedCase:
    """Tensors of a planted masked case (CPU) plus what the tests need to
    know about it: winners[b] (-1 = nothing may answer) and the queries
    whose decoy out-scores the winner while ineligible."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def tensors(self):
        return (self.index, self.q, self.row_scope, self.row_expiry, self.q_scope,
                self.now)


def scoped_case(n_rows: int, dim: int, dtype, queries, seed: int,
                now: int = 1000) -> ScopedCase:
    """Planted masked inputs. Background: seeded unit rows tagged with the
    scopes of the call's own scoped queries, one row in eight dead. The
    query for winner w is normalize(index[w] + 0.5 * unit noise), quantised:
    ~0.9 on its winner, <= ~0.43 on any other background row. A decoy is a
    copy of the quantised query (score |q|^2) under a tag that makes it
    ineligible. Every row has at most one role per call."""
    g = torch.Generator().manual_seed(seed + 7919)  # not unit_rows' stream
    index = unit_rows(n_rows, dim, dtype, seed).to(torch.float32)
    n_q = len(queries)
    roles = {}

    def claim(r, what):
        assert r is not None and 0 <= r < n_rows, (what, r, n_rows)
        assert r not in roles, f"row {r}: {what} collides with {roles[r]}"
        roles[r] = what

    for b, sp in enumerate(queries):
        if sp.winner is not None:
            claim(sp.winner, f"winner of query {b}")
        if sp.decoy is not None:
            claim(sp.decoy, f"decoy of query {b}")
        if sp.runner is not None:
            claim(sp.runner, f"runner-up of query {b}")
    # background tags: scopes shared with the queries, so each scoped query
    # has eligible background rows besides its winner
    shared = [sp.scope for sp in queries
              if sp.scope != 0 and sp.winner is not None and not sp.negative]
    if not shared:
        shared = scope_ids(3, seed + 1)
    pick = torch.randint(0, len(shared), (n_rows,), generator=g).tolist()
    row_scope = [shared[i] for i in pick]
    row_expiry = [min(now + 1 + int(v), NEVER) for v in
                  torch.randint(0, 50, (n_rows,), generator=g).tolist()]
    dead = (now, now - 1, min(now, 0), INT32_MIN)
    for r in range(n_rows):
        if r % 7 == 3:
            row_expiry[r] = NEVER
        if r % 8 == 5:
            row_expiry[r] = dead[(r // 8) % 4]
    noise = torch.nn.functional.normalize(torch.randn(n_q, dim, generator=g), dim=1)
    q = torch.empty(n_q, dim)
    for b, sp in enumerate(queries):
        anchor = sp.winner if (sp.winner is not None and not sp.negative) else None
        base = index[anchor] if anchor is not None else torch.zeros(dim)
        v = torch.nn.functional.normalize(base + (0.5 if anchor is not None else 1.0)
                                          * noise[b], dim=0)
        q[b] = v.to(torch.bfloat16).to(dtype).to(torch.float32)
    winners, shadowed = [], []
    for b, sp in enumerate(queries):
        winners.append(-1 if sp.winner is None else sp.winner)
        if sp.winner is not None:
            if sp.negative:
                index[sp.winner] = -0.5 * q[b]
                index[sp.runner] = -q[b]
                row_scope[sp.runner], row_expiry[sp.runner] = sp.scope, NEVER
            row_scope[sp.winner] = sp.scope if sp.scope != 0 else row_scope[sp.winner]
            row_expiry[sp.winner] = (sp.winner_expiry if sp.winner_expiry is not None
                                     else (min(now + 1, NEVER), NEVER)[b % 2])
        if sp.decoy is not None:
            index[sp.decoy] = q[b]
            row_scope[sp.decoy], row_expiry[sp.decoy] = sp.decoy_scope, sp.decoy_expiry
            eligible = sp.decoy_expiry > now and sp.scope in (0, sp.decoy_scope)
            if sp.winner is not None and not eligible:
                shadowed.append(b)
    return ScopedCase(
        index=index.to(torch.bfloat16).to(dtype),
        q=q.to(torch.bfloat16).to(dtype),
        row_scope=torch.tensor(row_scope, dtype=torch.int64),
        row_expiry=torch.tensor(row_expiry, dtype=torch.int32),
        q_scope=torch.tensor([sp.scope for sp in queries], dtype=torch.int64),
        now=now, winners=winners, shadowed=shadowed)


def pair_queries(winners, scopes, n_rows, now, kinds=DECOY_KINDS, start=0):
    """One ScopedQuery per winner with its decoy at the pair partner w ^ 1
    (same 4-row lane group, below an odd winner and above an even one) where
    that row exists; decoy kinds and foreign-scope variants cycle."""
    out = []
    for i, (w, s) in enumerate(zip(winners, scopes)):
        d = w ^ 1
        k = start + i
        out.append(scoped_query(w, s, d if d < n_rows else None,
                                kinds[k % len(kinds)], now, k // len(kinds)))
    return out


# ---------------------------------------------------------------------------
# gemm_bf16_nt
# ---------------------------------------------------------------------------

def gemm_reference(a, bt, bias, relu):
    """fp64 reference and elementwise fp32-accumulation bound:
    K * 2^-23 * (|a| @ |bt|^T) + 2^-23 * |ref|."""
    a64 = a.detach().cpu().to(torch.float64)
    b64 = bt.detach().cpu().to(torch.float64)
    ref = a64 @ b64.T
    if bias is not None:
        ref = ref + bias.detach().cpu().to(torch.float64)[None, :]
    if relu:
        ref = torch.relu(ref)
    k = a64.shape[1]
    bound = k * EPS23 * (a64.abs() @ b64.abs().T) + EPS23 * ref.abs()
    return ref, bound


def check_gemm(c, a, bt, bias, relu) -> dict:
    ref, bound = gemm_reference(a, bt, bias, relu)
    got = c.detach().cpu().to(torch.float64)
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), "non-finite GEMM output"
    err = (got - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    bad = err > bound
    if bad.any():
        i, j = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError(
            f"{int(bad.sum())} of {bad.numel()} elements out of bound; first "
            f"at ({i},{j}): got {float(got[i, j])!r} want {float(ref[i, j])!r} "
            f"|err| {float(err[i, j]):.3e} > {float(bound[i, j]):.3e}")
    return {"max_err": float(err.max()), "max_err_over_bound": float(ratio.max())}


def gemm_inputs(m: int, n: int, k: int, seed: int, with_bias: bool):
    """Asymmetric random bf16 operands with a loud tail: the last 8 K
    columns, the last row of a and the last row of bt are ~10x the scale
    of the rest, so an error confined to a tail cannot hide in the noise."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(m, k, generator=g) + 0.25
    bt = torch.randn(n, k, generator=g) - 0.125
    a[:, k - 8:] = 10.0 * torch.randn(m, 8, generator=g) + 3.0
    bt[:, k - 8:] = 10.0 * torch.randn(n, 8, generator=g) - 2.0
    a[m - 1, :] = 10.0 * torch.randn(k, generator=g) + 1.0
    bt[n - 1, :] = 10.0 * torch.randn(k, generator=g) - 1.5
    bias = None
    if with_bias:
        bias = 50.0 * torch.randn(n, generator=g)
    return a.to(torch.bfloat16), bt.to(torch.bfloat16), bias


def emulate_gemm(a, bt, bias, relu):
    """Pure-torch fp32 emulation of gemm_bf16_nt's contract."""
    c = a.to(torch.float32) @ bt.to(torch.float32).T
    if bias is not None:
        c = c + bias.to(torch.float32)[None, :]
    return torch.relu(c) if relu else c


# ---------------------------------------------------------------------------
# kv_score_assign
# ---------------------------------------------------------------------------

KV_WEIGHTS = (1.0, 0.125, 0.0625)


def kv_greedy_ref(stats, pred, weights, dtype, penalty=True) -> list[int]:
    """Greedy assignment reference evaluated in `dtype` (np.float32 or
    np.float64): score = w_kv*(1 - (used+p)/max(total,1)) - w_q*queue -
    w_a*active, minus 1e6 when used+p exceeds the replica's capacity;
    argmax with the lowest index winning ties; the winner absorbs p."""
    f = dtype
    s = np.array(stats, dtype=f).copy()
    w_kv, w_q, w_a = (f(w) for w in weights)
    out = []
    for p in np.asarray(pred, dtype=f):
        best, best_score = -1, None
        for r in range(s.shape[0]):
            used, total, queue, active = s[r]
            sc = w_kv * (f(1) - (used + p) / max(total, f(1))) - w_q * queue - w_a * active
            if penalty and used + p > total:
                sc = sc - f(1e6)
            if best_score is None or sc > best_score:
                best, best_score = r, sc
        out.append(best)
        s[best, 0] += p
        s[best, 2] += f(1)
        s[best, 3] += f(1)
    return out


def kv_cases(n_req: int = 200) -> dict:
    """name -> (stats rows, pred). All values are integers and every
    kv_total is a power of two (or zero), so with KV_WEIGHTS every
    intermediate of the score is exact in fp32; tests assert that by
    comparing the fp32 and fp64 references before trusting either."""
    rng = np.random.default_rng(20)
    cases = {}
    pred = rng.integers(1, 48, n_req).astype(np.float64)
    for n_rep in (1, 2, 63, 64):
        # identical replicas: every request starts from an exact tie
        cases[f"identical_{n_rep}"] = (
            [[0.0, 65536.0, 0.0, 0.0] for _ in range(n_rep)], pred)
        # mixed load, one zero-capacity replica (never eligible while any
        # other replica fits), one full replica the penalty must
        # steer away from
        # (penalised scores are not exact here, so at least one replica must
        # always fit: capacities are >= 2^14 against ~5000 tokens in total;
        # only n_rep == 1 is all-penalised, and there integers stay exact)
        rows = []
        for r in range(n_rep):
            total = float(2 ** int(rng.integers(14, 17)))
            rows.append([float(rng.integers(0, int(total) // 2)), total,
                         float(rng.integers(0, 7)), float(rng.integers(0, 7))])
        rows[0] = [0.0, 0.0, 0.0, 0.0]
        if n_rep > 2:
            rows[n_rep - 1] = [8192.0, 8192.0, 0.0, 0.0]
        cases[f"mixed_{n_rep}"] = (rows, pred)
        # all replicas overflow from the first request on: kv_total = 16 and
        # pred >= 17, so every score carries the -1e6 penalty and stays a
        # multiple of 2^-4 (the fp32 spacing just below 2^20)
        rows = [[float(rng.integers(0, 17)), 16.0, float(rng.integers(0, 4)),
                 float(rng.integers(0, 4))] for _ in range(n_rep)]
        cases[f"all_overflow_{n_rep}"] = (
            rows, rng.integers(17, 48, n_req).astype(np.float64))
    return cases


# ---------------------------------------------------------------------------
# BPE
# ---------------------------------------------------------------------------

_LETTERS = b"etaoinshr"


def _letters(n, seed):
    rng = np.random.default_rng(seed)
    return bytes(_LETTERS[int(i)] for i in rng.integers(0, len(_LETTERS), n))


def _prose(n, seed):
    rng = np.random.default_rng(seed)
    alphabet = b"etaoinshr 0123.,!\n\xc3\xa9"
    return bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), n))


def _group_text(last_len):
    """One request whose first group (segment starts 0,5,..,30, all in the
    first 32-byte cell) ends exactly at byte 30 + last_len, where the next
    group starts: sE - s0 = 64 packs the last segment into the wave window,
    65 sends it down the single-segment path."""
    head = b"etaoi" + b" nshr" * 5          # segments start at 0,5,10,15,20,25
    last = b" " + _letters(last_len - 1, 9)  # starts at 30
    return head + last + b" tail end"


def bpe_cases() -> dict:
    """name -> list of request texts for the BPE edge tests."""
    cases = {
        "total_255": [_prose(100, 1), _prose(80, 2), _prose(75, 3)],
        "total_256": [_prose(100, 4), _prose(80, 5), _prose(76, 6)],
        "total_257": [_prose(100, 7), _prose(80, 8), _prose(77, 9)],
        "total_512": [_prose(200, 10), _prose(56, 11), _prose(256, 12)],
        "boundary_at_256": [_letters(250, 13) + b" hello", b"world " + _prose(94, 14)],
        "boundary_inside_segments": [b"hel", b"lo wor", b"ld"],
        "segments_63_64_65_128_129": [_letters(n, n) for n in (63, 64, 65, 128, 129)],
        "segment_64_alone": [_letters(64, 164)],
        "segment_65_alone": [_letters(65, 165)],
        "segment_129_alone": [_letters(129, 229)],
        "group_span_64": [_group_text(34)],
        "group_span_65": [_group_text(35)],
        "tiny_600": [_prose(1 + i % 3, 300 + i) for i in range(600)],
        "seeded_200": [_prose(int(n), 1000 + i) for i, n in enumerate(
            np.random.default_rng(15).integers(1, 301, 200))],
    }
    # the same texts behind a 13-byte first request: every 32-byte cell and
    # 64-byte chunk is then unaligned to the byte buffer
    for name in ("boundary_inside_segments", "segments_63_64_65_128_129",
                 "group_span_64", "group_span_65", "total_256"):
        cases[name + "_behind_13"] = [b"thirteen byte"] + cases[name]
    # empty texts (the force-starts kernel skips req_off >= n, as the
    # oracle's segment_starts does)
    cases.update({
        "empty_leading": [b"", b"hello world", b"again"],
        "empty_middle": [b"hello wor", b"", b"", b"ld again"],
        "empty_trailing": [b"hello world", b"x", b""],
        "empty_all_but_one": [b"", b"", b"only this one", b"", b""],
        "empty_trailing_total_512": [_prose(256, 16), _prose(256, 17), b"", b""],
    })
    return cases


# ---------------------------------------------------------------------------
# native admission path (aigw_fast.AdmissionProbe)
# ---------------------------------------------------------------------------

PROBE_DIM = 384
PROBE_N_MERGES = 8192
PROBE_SEED = 1355


def probe_lookup_texts(n: int = 130) -> list[bytes]:
    """Distinct seeded texts, 1..60 words each, every text over its own
    small word set so that no two texts embed close together."""
    out = []
    for i in range(n):
        rng = np.random.default_rng(5000 + i)
        words = [_letters(int(rng.integers(2, 9)), 9000 + 31 * i + w)
                 for w in range(6)]
        k = int(rng.integers(1, 61))
        out.append(b" ".join(words[int(j)] for j in rng.integers(0, 6, k))
                   + b" %d" % i)
    return out


def probe_big_batch(lookup_texts: list[bytes]) -> list[bytes]:
    """300 texts, > 66 000 bytes: 170 fillers (1-byte texts included) in
    front of the lookup texts, so both the 256-byte-block scan and the
    per-request scan carry across more than one 256-entry chunk and the
    lookup texts sit behind the carry."""
    fillers = []
    for i in range(170):
        if i % 10 == 0:
            fillers.append(_prose(1, 700 + i))
        else:
            fillers.append(_prose(200 + (i * 37) % 500, 700 + i))
    return fillers + list(lookup_texts)


def probe_weights(vocab: int, seed: int = 7):
    """Random-init bf16 embedding table and projection (same recipe as
    aigw.ops.semcache)."""
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(vocab, PROBE_DIM, generator=g).to(torch.bfloat16)
    proj = (torch.randn(PROBE_DIM, PROBE_DIM, generator=g) / PROBE_DIM ** 0.5).to(
        torch.bfloat16)
    return emb, proj


def probe_reference(ids_list, emb, proj, fp8: bool, dtype=torch.float64):
    """The native embed pipeline evaluated in `dtype`, mirroring every
    rounding stage: mean of the bf16 token rows -> bf16 -> projection ->
    x * rsqrt(sum x^2 + 1e-12) -> bf16 -> (e4m3 for the fp8 index).
    Returns the (B, dim) query matrix in `dtype` (values exactly
    representable in the index format)."""
    e = emb.to(dtype)
    p = proj.to(dtype)
    rows = []
    for ids in ids_list:
        t = torch.as_tensor(ids, dtype=torch.long)
        pooled = e[t].mean(dim=0).to(torch.float32).to(torch.bfloat16).to(dtype)
        g = p @ pooled
        qv = g * torch.rsqrt((g * g).sum() + 1e-12)
        qv = qv.to(torch.float32).to(torch.bfloat16)
        if fp8:
            qv = qv.to(torch.float8_e4m3fn)
        rows.append(qv.to(dtype))
    return torch.stack(rows)


def probe_plain_fp32(ids_list, emb, proj, fp8: bool):
    """The same stages as a plain batched torch fp32 evaluation (no fp64
    anywhere, one matmul for the whole batch): the yardstick for how far
    an honest fp32 pipeline may land from the fp64 mirrored reference when
    a value sits on a bf16/e4m3 rounding boundary."""
    pooled = torch.stack([emb[torch.as_tensor(i, dtype=torch.long)].float().mean(dim=0)
                          for i in ids_list]).to(torch.bfloat16)
    g = pooled.float() @ proj.float().T
    qv = (g * torch.rsqrt((g * g).sum(dim=1, keepdim=True) + 1e-12)).to(torch.bfloat16)
    if fp8:
        qv = qv.to(torch.float8_e4m3fn)
    return qv.float()


# Largest |self-match score (plain fp32) - self-match score (fp64 mirrored
# reference)| over the probe_lookup_texts() inputs and both index formats,
# measured on the CPU: 4 of the 49 920 bf16 roundings land on the other
# side of a boundary, the worst moves a score by 2.51e-5 (fp8: none, 0.0).
# The lookup test allows 4x that for the kernel's own boundary flips.
PROBE_MEASURED_FP32_DISAGREEMENT = 2.52e-5
PROBE_SCORE_ALLOWANCE = 4 * PROBE_MEASURED_FP32_DISAGREEMENT


def probe_score_stats(ids_list, emb, proj, fp8: bool) -> dict:
    """fp64 mirrored reference vectors and self-match scores, their
    largest disagreement with the plain fp32 evaluation, and the smallest
    self-match lead over the best other text."""
    q64 = probe_reference(ids_list, emb, proj, fp8, torch.float64)
    q32 = probe_plain_fp32(ids_list, emb, proj, fp8)
    s64 = q64 @ q64.T
    self64 = s64.diagonal().clone()
    self32 = (q32 * q32).sum(dim=1).to(torch.float64)
    measured = float((self32 - self64).abs().max())
    off = s64.clone()
    off.fill_diagonal_(-float("inf"))
    lead = float((self64 - off.max(dim=1).values).min())
    return {"q": q64, "self": self64, "measured": measured, "min_lead": lead}
