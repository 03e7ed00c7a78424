"""Scope- and TTL-filtered cache lookup (cache_topk_scoped) against the fp64
product of the same quantised tensors: scores.masked_fill(~eligible, -inf).
Values are held to the a-priori fp32 dot-product bound of
tests/kernel_checks.py, dim * 2^-23 * |row| * |q|; that the returned row is
eligible is exact, not a tolerance. These inputs are random, so two rows may
score within the bound of each other and the row itself is not compared
(tests/test_gpu_cache_scoped_edges.py does that on planted inputs)."""

import pytest
import torch

from kernel_checks import EPS23

pytestmark = pytest.mark.gpu

NEVER = 0x7FFFFFFF
DTYPES = [torch.bfloat16, torch.float8_e4m3fn]


@pytest.fixture(scope="module")
def hip():
    import aigw_hip

    return aigw_hip


def _unit(n, dim, gen):
    v = torch.randn(n, dim, generator=gen, device="cuda")
    return torch.nn.functional.normalize(v, dim=1).to(torch.bfloat16)


def _i64(x):
    return torch.as_tensor(x, dtype=torch.int64, device="cuda")


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32, device="cuda")


def _eligible(row_scope, row_expiry, q_scope, now):
    live = (row_expiry > now)[:, None]
    match = (q_scope == 0)[None, :] | (row_scope[:, None] == q_scope[None, :])
    return live & match  # (n_rows, n_q)


def _check_against_reference(hip, index, q, row_scope, row_expiry, q_scope, now):
    """Runs the op and checks every query: no eligible row <-> idx -1 / hi 0;
    otherwise the row is eligible, the returned score is within the bound
    of the masked fp64 maximum, and the returned row's exact score within
    twice the bound (the kernel's own error on that row plus its error on
    the true argmax). The bound takes the largest row norm, so it holds
    whichever row came back."""
    from aigw.ops.semcache import _unorder

    hi, idx = hip.cache_topk_scoped(index, q, row_scope, row_expiry, q_scope, now)
    index64, q64 = index.cpu().to(torch.float64), q.cpu().to(torch.float64)
    scores = index64 @ q64.t()
    elig = _eligible(row_scope, row_expiry, q_scope, now).cpu()
    ref_val = scores.masked_fill(~elig, float("-inf")).max(dim=0).values
    bound = index.shape[1] * EPS23 * float(index64.norm(dim=1).max()) * q64.norm(dim=1)
    hi, idx = hi.cpu().tolist(), idx.cpu().tolist()
    for b in range(q.shape[0]):
        if not bool(elig[:, b].any()):
            assert idx[b] == -1 and hi[b] == 0, (b, idx[b], hi[b])
            continue
        assert 0 <= idx[b] < index.shape[0], (b, idx[b])
        assert bool(elig[idx[b], b]), (b, idx[b])
        got, want, tol = _unorder(hi[b]), float(ref_val[b]), float(bound[b])
        assert abs(got - want) <= tol, (b, got, want, tol)
        assert abs(float(scores[idx[b], b]) - want) <= 2 * tol, (b, idx[b], tol)
    return idx


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp8"])
@pytest.mark.parametrize("dim", [128, 384])
@pytest.mark.parametrize("n_q", [1, 17, 129])
def test_masked_argmax_shapes(hip, dtype, dim, n_q):
    """5 blocks with a partial last tile; a quarter of the rows expired;
    every fourth query wildcard; the last query's scope matches nothing."""
    gen = torch.Generator(device="cuda").manual_seed(dim * 1000 + n_q)
    n_rows, now = 4100, 1000
    index = _unit(n_rows, dim, gen).to(dtype)
    q = _unit(n_q, dim, gen).to(dtype)
    row_scope = torch.randint(1, 6, (n_rows,), generator=gen, device="cuda")
    row_expiry = torch.randint(now + 1, now + 50, (n_rows,), generator=gen,
                               device="cuda", dtype=torch.int32)
    dead = torch.rand(n_rows, generator=gen, device="cuda") < 0.25
    row_expiry[dead] = torch.randint(0, now + 1, (n_rows,), generator=gen, device="cuda",
                                     dtype=torch.int32)[dead]
    row_expiry[::7] = NEVER
    q_scope = torch.randint(1, 6, (n_q,), generator=gen, device="cuda")
    q_scope[::4] = 0
    q_scope[n_q - 1] = 99
    idx = _check_against_reference(hip, index, q, row_scope, row_expiry, q_scope, now)
    assert idx[n_q - 1] == -1
    assert all(i >= 0 for i in idx[:-1])
    if n_q == 1:  # the only query was the unmatched one: also run it matched
        for s in (0, 3):
            idx = _check_against_reference(hip, index, q, row_scope, row_expiry,
                                           _i64([s]), now)
            assert idx[0] >= 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp8"])
def test_duplicate_vector_under_three_scopes(hip, dtype):
    """The shadowing case: one vector stored under three scopes scores the
    same three times, so an unfiltered argmax serves one scope only. The
    three rows sit inside one lane's 4-row group (40..42), across a 16-row
    tile edge (30..32) and across the 1024-row block edge (1023..1025)."""
    gen = torch.Generator(device="cuda").manual_seed(11)
    dim, n_rows = 384, 2100
    index = _unit(n_rows, dim, gen)
    vecs = _unit(3, dim, gen)
    firsts = [40, 30, 1023]
    scopes = [11, 12, 13]
    row_scope = torch.randint(1, 6, (n_rows,), generator=gen, device="cuda")
    for k, r0 in enumerate(firsts):
        for j in range(3):
            index[r0 + j] = vecs[k]
            row_scope[r0 + j] = scopes[j]
    row_expiry = torch.full((n_rows,), NEVER, dtype=torch.int32, device="cuda")
    # per placement: one query per scope, then the wildcard
    q = vecs.repeat_interleave(4, dim=0).to(dtype)
    q_scope = _i64((scopes + [0]) * 3)
    _, idx = hip.cache_topk_scoped(index.to(dtype), q, row_scope, row_expiry, q_scope, 5)
    idx = idx.cpu().tolist()
    for k, r0 in enumerate(firsts):
        assert idx[4 * k : 4 * k + 3] == [r0, r0 + 1, r0 + 2], (k, idx)
        # wildcard: all three tie, the highest row wins (pack_score's rule)
        assert idx[4 * k + 3] == r0 + 2, (k, idx)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp8"])
def test_expiry_edge(hip, dtype):
    gen = torch.Generator(device="cuda").manual_seed(23)
    dim, n_rows, now = 128, 2100, 500
    index = _unit(n_rows, dim, gen)
    qv = _unit(2, dim, gen)
    row_scope = torch.randint(1, 6, (n_rows,), generator=gen, device="cuda")
    row_expiry = torch.full((n_rows,), now + 1, dtype=torch.int32, device="cuda")
    # expiry == now is dead, now + 1 alive: of two copies the dead one would
    # win the tie (higher row)
    index[5] = qv[0]
    index[6] = qv[0]
    row_expiry[6] = now
    # a tile whose 16 rows are all dead, holding query 1's exact match
    index[70] = qv[1]
    row_expiry[64:80] = now - 1
    index, q = index.to(dtype), qv.to(dtype)
    q_scope = _i64([0, 0])
    idx = _check_against_reference(hip, index, q, row_scope, row_expiry, q_scope, now)
    assert idx[0] == 5
    assert not 64 <= idx[1] < 80
    # entirely dead index: nothing for anybody
    hi, idx = hip.cache_topk_scoped(index, q, row_scope, torch.full_like(row_expiry, now),
                                    q_scope, now)
    assert idx.cpu().tolist() == [-1, -1] and hi.cpu().tolist() == [0, 0]


def test_tag_tensor_checks(hip):
    gen = torch.Generator(device="cuda").manual_seed(1)
    index, q = _unit(64, 128, gen), _unit(2, 128, gen)
    rs, re, qs = _i64([1] * 64), _i32([NEVER] * 64), _i64([0, 0])
    hip.cache_topk_scoped(index, q, rs, re, qs, 0)
    for bad in [
        (index, q, rs[:63], re, qs),  # shape
        (index, q, rs.to(torch.int32), re, qs),  # dtype
        (index, q, rs, re.to(torch.int64), qs),
        (index, q, rs, re, qs[:1]),
        (index, q, rs.cpu(), re, qs),  # device
    ]:
        with pytest.raises(RuntimeError):
            hip.cache_topk_scoped(*bad, 0)


@pytest.mark.parametrize("index_dtype", ["bf16", "fp8"])
def test_semantic_cache_scoped_end_to_end(hip, index_dtype):
    from aigw.ops.semcache import SemanticCache
    from aigw.ops.tokenizer import GPUTokenizer

    tok = GPUTokenizer(n_merges=4096, device="cuda")
    t = [0.0]
    kw = dict(threshold=0.95, device="cuda", index_dtype=index_dtype, scoped=True,
              _clock=lambda: t[0])
    cache = SemanticCache(tok.vocab_size, capacity=64, **kw)
    texts = [b"what is the capital of france", b"how do i cook rice",
             b"unrelated database question"]
    _, _, state = tok.encode_batch(texts)
    vecs = cache.embed(state["out_ids"], state["req_off"])
    a, b = cache.scope_id(b"tenant-a"), cache.scope_id(b"tenant-b")

    def value(i, scope):
        hit = cache.lookup(vecs[i : i + 1], scopes=[scope])[0]
        return None if hit is None else cache.get(hit[0])

    cache.insert(vecs[0], b"A-PARIS", scope=a)
    assert value(0, a) == b"A-PARIS" and value(0, b) is None
    # the same text under a second scope: each scope gets its own row back
    # (an unfiltered argmax returns one row for both, so one always misses)
    cache.insert(vecs[0], b"B-PARIS", scope=b)
    assert value(0, a) == b"A-PARIS" and value(0, b) == b"B-PARIS"
    assert [cache.get(h[0]) for h in cache.lookup(vecs[[0, 0]], scopes=[b, a])] == [
        b"B-PARIS", b"A-PARIS"]

    cache.insert(vecs[1], b"A-RICE", scope=a, ttl_s=10)
    t[0] = 9.0
    assert value(1, a) == b"A-RICE"
    t[0] = 10.0
    assert value(1, a) is None
    assert value(0, a) == b"A-PARIS"  # no TTL: still there

    assert cache.invalidate(scope=a) == 2
    assert value(0, a) is None and value(0, b) == b"B-PARIS"
    assert cache.invalidate() == 1 and value(0, b) is None

    # ring wrap: the overwritten slot takes the new row's tag
    ring = SemanticCache(tok.vocab_size, capacity=4, **kw)
    assert ring.insert(vecs[0], b"OLD", scope=a) == 0
    for i in (1, 2, 1):
        ring.insert(vecs[i], b"FILL", scope=a)
    assert ring.insert(vecs[0], b"NEW", scope=b) == 0
    hit_a, hit_b = ring.lookup(vecs[[0, 0]], scopes=[a, b])
    assert hit_a is None
    assert hit_b is not None and hit_b[0] == 0 and ring.get(0) == b"NEW"


@pytest.mark.parametrize("index_dtype", ["bf16", "fp8"])
def test_unscoped_default_is_cache_topk(hip, index_dtype):
    from aigw.ops.semcache import SemanticCache, _unorder

    gen = torch.Generator(device="cuda").manual_seed(5)
    cache = SemanticCache(512, dim=128, capacity=64, threshold=-2.0, device="cuda",
                          index_dtype=index_dtype)
    rows = _unit(40, 128, gen)
    for i in range(40):
        cache.insert(rows[i], b"v%d" % i)
    q = _unit(9, 128, gen)
    hi, idx = hip.cache_topk(cache.index[:40], q.to(cache.index_dtype))
    want = [(i, _unorder(h)) for h, i in zip(hi.cpu().tolist(), idx.cpu().tolist())]
    assert cache.lookup(q) == want
