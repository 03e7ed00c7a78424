"""cache_topk_k against the fp64 product sorted by (score, row) descending.
Inputs are integers in {-2..2}, exact in bf16, e4m3 and the fp32 accumulator,
so rows and scores are compared exactly."""

import asyncio
import functools

import pytest
import torch

from aigw.ops.semcache import SemanticCache, _unorder

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float8_e4m3fn],
                                 ids=["bf16", "fp8"])
N_ROWS = 1103  # 1024 + 64 + 15: two blocks, a partial last tile ending in a 3-row group
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
    """Per query: [(row, score)] of every eligible row, best first."""
    s = index.double() @ q.double().T
    ok = torch.ones_like(s, dtype=torch.bool)
    if tags is not None:
        rs, re, qs = tags
        ok = (re > NOW)[:, None] & ((qs == 0)[None, :] | (rs[:, None] == qs[None, :]))
    out = []
    for b in range(q.shape[0]):
        col, okb = s[:, b].tolist(), ok[:, b].tolist()
        rows = sorted((r for r in range(len(col)) if okb[r]),
                      key=lambda r: (col[r], r), reverse=True)
        out.append([(r, col[r]) for r in rows])
    return out


@functools.lru_cache(maxsize=None)
def _shape_reference(n_rows, n_q, dim, scoped):
    index, q, *tags = _inputs(n_rows, n_q, dim)
    return _reference(index, q, tags if scoped else None)


def _check(hip, index, q, k, dtype, tags=None, want=None):
    """Runs the op and compares idx and the decoded scores exactly; returns idx."""
    args = [index.to(dtype).cuda(), q.to(dtype).cuda(), k]
    if tags is not None:
        args += [t.cuda() for t in tags] + [NOW]
    hi, idx = (t.cpu().tolist() for t in hip.cache_topk_k(*args))
    for b, w in enumerate(want or _reference(index, q, tags)):
        w = w[:k]
        pad = k - len(w)
        assert idx[b] == [r for r, _ in w] + [-1] * pad, (b, idx[b], w)
        assert [_unorder(h) for h in hi[b][:len(w)]] == [s for _, s in w], (b, hi[b], w)
        assert hi[b][len(w):] == [0] * pad, (b, hi[b])
    return idx


def test_reference_tie_order():
    index = torch.tensor([[1.0], [3.0], [3.0], [2.0]])
    assert _reference(index, torch.ones(1, 1)) == [[(2, 3.0), (1, 3.0), (3, 2.0), (0, 1.0)]]


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("dim", [128, 256, 384, 512])  # bf16 512: 64-query passes
@pytest.mark.parametrize("n_q", [1, 17, 129])
@pytest.mark.parametrize("n_rows", [1, 17, N_ROWS])
@DTYPES
def test_shapes(hip, dtype, n_rows, n_q, dim, k):
    index, q, *tags = _inputs(n_rows, n_q, dim)
    _check(hip, index, q, k, dtype, want=_shape_reference(n_rows, n_q, dim, False))
    _check(hip, index, q, k, dtype, tags, _shape_reference(n_rows, n_q, dim, True))


@DTYPES
def test_k1_is_the_argmax_kernels_key(hip, dtype):
    index, q, *tags = _inputs(N_ROWS, 129, 384)
    # cache_topk gives an exact tie inside an aligned group of four rows to
    # the lower row, cache_topk_k to the higher: the inputs must hold no such
    # tie for a best score, or the comparison would not be of equals
    assert all(w[0][1] != w[1][1] or w[0][0] // 4 != w[1][0] // 4
               for w in _shape_reference(N_ROWS, 129, 384, False))
    index, q, *tags = (t.cuda() for t in (index.to(dtype), q.to(dtype), *tags))
    for got, want in ((hip.cache_topk_k(index, q, 1), hip.cache_topk(index, q)),
                      (hip.cache_topk_k(index, q, 1, *tags, NOW),
                       hip.cache_topk_scoped(index, q, *tags, NOW))):
        assert torch.equal(got[0].flatten(), want[0]) and torch.equal(got[1].flatten(), want[1])


# a lane group (40, 41), waves 1 and 2 of block 0, block 1, the last partial
# tile (1088..1102) and its 3-row group (1100..1102)
COPIES = [40, 41, 300, 600, 1030, 1090, 1100, 1102]


@pytest.mark.parametrize("scoped", [False, True])
@pytest.mark.parametrize("k", [3, 8])
@DTYPES
def test_ties_and_two_rows_of_one_lane(hip, dtype, k, scoped):
    """Query 0 has 8 exact copies of its best row across the structure;
    query 1's two best rows, 520 and 521, sit in one lane's four rows."""
    index, q, *_ = (t.clone() for t in _inputs(N_ROWS, 2, 128))
    q[q == 0] = 1.0  # |q|^2 >= dim: well above any random row
    index[COPIES], index[520], index[521] = q[0], q[1], q[1]
    index[521, 0] = 0.0
    tags = None
    if scoped:  # every row live, one scope; a scoped and a wildcard query
        tags = (torch.full((N_ROWS,), 5), torch.full((N_ROWS,), NOW + 1).int(),
                torch.tensor([5, 0]))
    idx = _check(hip, index, q, k, dtype, tags)
    assert idx[0] == sorted(COPIES, reverse=True)[:k] and idx[1][:2] == [520, 521]


@pytest.mark.parametrize("k", [3, 8])
@DTYPES
def test_mask(hip, dtype, k):
    index, q, row_scope, row_expiry, _ = (t.clone() for t in _inputs(N_ROWS, 4, 128))
    q[q == 0] = 1.0
    q[2] = index[10] = index[11] = q[0]  # rows 10, 11 out-score every other row
    row_scope[10], row_expiry[10] = 9, NOW + 1  # foreign to query 0's scope 5
    row_scope[11], row_expiry[11] = 5, NOW  # its scope, but expired
    row_scope[700], row_expiry[700] = 33, NOW + 1  # query 3's only two rows
    row_scope[1101], row_expiry[1101] = 33, NOW + 1
    tags = (row_scope, row_expiry, torch.tensor([5, 77, 0, 33]))
    idx = _check(hip, index, q, k, dtype, tags)
    assert 10 not in idx[0] and 11 not in idx[0] and -1 not in idx[0]
    assert idx[1] == [-1] * k
    assert idx[2][0] == 10 and 11 not in idx[2]  # wildcard: all live rows
    assert sorted(idx[3][:2]) == [700, 1101] and idx[3][2:] == [-1] * (k - 2)


def test_python_surface(hip):
    cache = SemanticCache(100, dim=128, capacity=64, device="cuda", _hip=hip)
    g = torch.Generator().manual_seed(3)
    v = torch.nn.functional.normalize(torch.randn(4, 128, generator=g), dim=1).cuda()
    # Duplicates at slots 3 and 4, two lane groups: the unfiltered arg-max
    # gives an exact tie inside one lane's four rows to the lower row.
    slots = [cache.insert(x, b"v") for x in (v[1], v[2], v[3], v[0], v[0])][3:]
    found = cache.lookup_k(v[:1], 2)[0]
    assert [s for s, _ in found] == slots[::-1]
    assert all(abs(score - 1.0) < 0.02 for _, score in found)
    assert cache.lookup(v[:1])[0][0] == slots[1]
    mx = SemanticCache(100, dim=128, capacity=64, device="cuda", _hip=hip,
                       index_dtype="mxfp4")
    with pytest.raises(ValueError, match="mxfp4"):
        mx.lookup_k(v[:1], 2)


def test_services_return_every_candidate():
    from aigw.gpu import GPUServices

    async def main(text=b"the same prompt twice"):
        gpu = GPUServices(device="cuda", n_merges=8192, enable_cache=True,
                          cache_capacity=64, cache_candidates=2)
        try:
            _, vec = await gpu.cache_lookup_text(text)
            await gpu.cache_insert(vec, b"A")
            await gpu.cache_insert(vec, b"B")
            assert (await gpu.cache_lookup_text_k(text))[0] == [b"B", b"A"]
            assert (await gpu.cache_lookup_text(text))[0] == b"B"
        finally:
            gpu.close()

    asyncio.run(main())
