"""cache_topk_wide_tiled against the fp64 product's maximum under (score, row)
order. Inputs are integers, exact in bf16 and e4m3, and sums stay at or under
4 * 2048, exact in fp32, so rows and decoded scores are compared exactly."""

import functools

import pytest
import torch

from aigw.ops.semcache import SemanticCache, _unorder

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float8_e4m3fn],
                                 ids=["bf16", "fp8"])
SCOPED = pytest.mark.parametrize("scoped", [False, True])
# 8 * 128 + 79: several 128-row blocks, a last block with two full waves, a
# wave ending in a partial tile whose last lane group has 3 rows, and a wave
# without rows
N_ROWS = 1103
NOW = 1000


@pytest.fixture(scope="module")
def hip():
    import aigw_hip

    return aigw_hip


@functools.lru_cache(maxsize=None)
def _inputs(n_rows, n_q, dim):
    """(index, q, row_scope, row_expiry, q_scope): a third of the rows dead
    (expiry == NOW), scopes 5/9, queries cycling wildcard, 5, 9, no-match."""
    g = torch.Generator().manual_seed(n_rows * 1000 + n_q * 10 + dim)
    index = torch.randint(-2, 3, (n_rows, dim), generator=g).float()
    q = torch.randint(-2, 3, (n_q, dim), generator=g).float()
    row_scope = torch.tensor([5, 9])[torch.randint(0, 2, (n_rows,), generator=g)]
    row_expiry = (NOW + torch.randint(0, 3, (n_rows,), generator=g)).int()
    return index, q, row_scope, row_expiry, torch.tensor([0, 5, 9, 77])[torch.arange(n_q) % 4]


def _reference(index, q, tags=None):
    """Per query: (row, score) of the eligible row with the largest
    (score, row), or (-1, None) when no row is eligible."""
    s = index.double() @ q.double().T
    ok = torch.ones_like(s, dtype=torch.bool)
    if tags is not None:
        rs, re, qs = tags
        ok = (re > NOW)[:, None] & ((qs == 0)[None, :] | (rs[:, None] == qs[None, :]))
    key = torch.where(ok, s, -torch.inf)
    best = key.max(dim=0).values
    # the highest row among those that reach the best score
    rows = (key == best).int().cumsum(0).argmax(0).tolist()
    return [(r, b) if b > -torch.inf else (-1, None) for r, b in zip(rows, best.tolist())]


@functools.lru_cache(maxsize=None)
def _shape_reference(n_rows, n_q, dim, scoped):
    index, q, *tags = _inputs(n_rows, n_q, dim)
    return _reference(index, q, tags if scoped else None)


def _check(hip, index, q, dtype, tags=None, want=None):
    """Runs the op and compares idx and the decoded scores exactly; returns idx."""
    args = [index.to(dtype).cuda(), q.to(dtype).cuda()]
    if tags is not None:
        args += [t.cuda() for t in tags] + [NOW]
    hi, idx = (t.cpu().tolist() for t in hip.cache_topk_wide_tiled(*args))
    want = want or _reference(index, q, tags)
    assert idx == [r for r, _ in want]
    assert [_unorder(h) if r >= 0 else h for h, r in zip(hi, idx)] == \
        [s if r >= 0 else 0 for r, s in want]
    return idx


# 640: 5 chunks in bf16, an odd count through the double buffer, and 2.5 in
# fp8; 2048: the most chunks. 129: the ninth query tile, the first of the
# stage's second half; 256: the full stage.
@pytest.mark.parametrize("dim", [640, 1024, 2048])
@pytest.mark.parametrize("n_q", [1, 17, 129, 256])
@pytest.mark.parametrize("n_rows", [1, 17, N_ROWS])
@DTYPES
def test_shapes(hip, dtype, n_rows, n_q, dim):
    index, q, *tags = _inputs(n_rows, n_q, dim)
    _check(hip, index, q, dtype, want=_shape_reference(n_rows, n_q, dim, False))
    idx = _check(hip, index, q, dtype, tags, _shape_reference(n_rows, n_q, dim, True))
    assert all(i == -1 for i in idx[3::4])  # scope 77 has no row


# the first five: blocks 0 and 2, wave 0 of block 8, and twice the partial
# last tile (1088..1102); 1100..1102 is its 3-row group
CAND = [40, 300, 1030, 1090, 1101, 3, 41, 130, 260, 515, 700, 1023, 1040, 1088, 1099, 1102]


@pytest.mark.parametrize("dim", [640, 2048])
@DTYPES
def test_every_chunk_meets_its_own_query_chunk(hip, dtype, dim):
    """Row CAND[c] is 1 on the 128 elements of chunk c; query j weighs chunk c
    by ((c + j) mod n) + 1. A dropped, repeated or mis-paired chunk on either
    operand (or half of a 256-element fp8 chunk) changes a winner or a score."""
    n = dim // 128
    index, q = torch.zeros(N_ROWS, dim), torch.zeros(n, dim)
    for c in range(n):
        index[CAND[c], c * 128:(c + 1) * 128] = 1.0
        for j in range(n):
            q[j, c * 128:(c + 1) * 128] = (c + j) % n + 1
    want = _reference(index, q)
    # every query has one best row: no tie decides a winner here
    scores = index.double() @ q.double().T
    assert all((scores[:, j] == s).sum() == 1 for j, (_, s) in enumerate(want))
    assert [r for r, _ in want] == [CAND[(n - 1 - j) % n] for j in range(n)]
    _check(hip, index, q, dtype, want=want)


@SCOPED
@DTYPES
def test_ties_go_to_the_higher_row(hip, dtype, scoped):
    """Query 0: two copies of its best row inside one lane's four rows;
    query 1: copies in three blocks, one of them in the partial tile."""
    index, q, *_ = (t.clone() for t in _inputs(N_ROWS, 2, 640))
    q[q == 0] = 1.0  # |q|^2 >= dim: well above any random row
    index[[40, 41]] = q[0]
    index[[130, 600, 1090]] = q[1]
    tags = None
    if scoped:
        tags = (torch.full((N_ROWS,), 5), torch.full((N_ROWS,), NOW + 1).int(),
                torch.tensor([5, 0]))
    assert _check(hip, index, q, dtype, tags) == [41, 1090]


@DTYPES
def test_mask(hip, dtype):
    """Queries 128..131 (wildcard, 5, 9, 77) sit in the upper half of the
    q_scope stage and of blk_best."""
    index, q, rs, re, qs = (t.clone() for t in _inputs(N_ROWS, 132, 640))
    q[q == 0] = 1.0
    index[[50, 300, 700]] = q[129]  # query 129 has scope 5
    index[50, 0] = 0.0              # second best, and the only one it may see
    rs[[50, 300, 700]] = torch.tensor([5, 9, 5])  # 300: foreign scope
    re[[50, 300, 700]] = torch.tensor([NOW + 1, NOW + 1, NOW], dtype=torch.int32)  # 700: expired
    index[900], rs[900], re[900] = q[128], 9, NOW + 1  # the wildcard sees any scope
    idx = _check(hip, index, q, dtype, (rs, re, qs))
    assert idx[128:] == [900, 50, idx[130], -1] and idx[130] >= 0
    assert _check(hip, index, q, dtype)[129] == 700  # unmasked: the higher copy


@SCOPED
@pytest.mark.parametrize("n_q", [129, 256])
@DTYPES
def test_same_key_as_the_multi_pass_op(hip, dtype, n_q, scoped):
    """The inputs do hold best-score ties (2 to 7 queries per case), and none
    is ambiguous: both ops give a tie to the higher row, which is the
    reference's order, so the rows are held against it here as well."""
    index, q, *tags = _inputs(N_ROWS, n_q, 1024)
    want = [r for r, _ in _shape_reference(N_ROWS, n_q, 1024, scoped)]
    args = [index.to(dtype).cuda(), q.to(dtype).cuda()]
    if scoped:
        args += [t.cuda() for t in tags] + [NOW]
    got, wide = hip.cache_topk_wide_tiled(*args), hip.cache_topk_wide(*args)
    assert torch.equal(got[0], wide[0]) and torch.equal(got[1], wide[1])
    assert got[1].cpu().tolist() == want


class _Spy:
    """The extension with the names of the ops called through it."""

    def __init__(self, hip):
        self.hip, self.calls = hip, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self.hip, name)


def _filled(hip, dim, index_dtype, n):
    cache = SemanticCache(100, dim=dim, capacity=256, device="cuda", _hip=_Spy(hip),
                          index_dtype=index_dtype)
    g = torch.Generator().manual_seed(dim)
    v = torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=1).cuda()
    slots = [cache.insert(x, b"v") for x in v]
    cache.hip.calls.clear()
    return cache, v, slots


def test_python_surface(hip):
    """dim 1024 is a width where the multi-pass op measured faster: lookup
    keeps it, and the results are the same."""
    cache, v, slots = _filled(hip, 1024, "fp8", 200)
    found = cache.lookup(v)
    assert [f[0] for f in found] == slots
    assert all(abs(f[1] - 1.0) < 0.02 for f in found)
    assert cache.lookup(v, scopes=[7] * 200) == [None] * 200
    assert "cache_topk_wide_tiled" not in cache.hip.calls


# shapes lookup hands to the new op, filtered or not: bf16 2048 from 2 passes,
# fp8 2048 with a full batch
@pytest.mark.parametrize("index_dtype,n", [("bf16", 130), ("fp8", 256)])
def test_lookup_through_the_tiled_op(hip, index_dtype, n):
    cache, v, slots = _filled(hip, 2048, index_dtype, n)
    for scopes in (None, [0] * n):  # [0] * n: the wildcard, through the mask
        cache.hip.calls.clear()
        found = cache.lookup(v, scopes=scopes)
        assert [f[0] for f in found] == slots
        assert all(abs(f[1] - 1.0) < 0.02 for f in found)
        assert "cache_topk_wide_tiled" in cache.hip.calls
        assert "cache_topk_wide" not in cache.hip.calls
    assert cache.lookup(v, scopes=[7] * n) == [None] * n


# (dtype, dim, queries, filtered) of the bold rows
SERVED = {("bf16", 768, 256, True), ("bf16", 1024, 256, True),
          *(("bf16", 1536, n, f) for n in (128, 256) for f in (False, True)),
          *(("bf16", 2048, n, f) for n in (37, 128, 256) for f in (False, True)),
          ("fp8", 1536, 128, True), ("fp8", 1536, 256, False), ("fp8", 1536, 256, True),
          ("fp8", 2048, 256, False), ("fp8", 2048, 256, True)}


def test_dispatch_is_the_profile_table(hip):
    """The bold rows of profiles/cache_topk_wide_tiled.md, and no other
    measured shape."""
    for index_dtype in ("bf16", "fp8"):
        for dim in (768, 1024, 1536, 2048):
            cache = SemanticCache(100, dim=dim, capacity=4, device="cuda", _hip=hip,
                                  index_dtype=index_dtype)
            for n_q in (37, 128, 256):
                for filtering in (False, True):
                    assert cache._wide_tiled_serves(n_q, filtering) == \
                        ((index_dtype, dim, n_q, filtering) in SERVED)
