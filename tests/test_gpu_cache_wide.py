"""cache_topk_wide against the fp64 product's maximum under (score, row)
order. Inputs are integers in {-2..2}, exact in bf16 and e4m3, and sums stay
at or under 4 * 2048, exact in fp32, so rows and decoded scores are compared
exactly."""

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
    """Per query: (row, score) of the eligible row with the largest
    (score, row), or (-1, None) when no row is eligible."""
    s = index.double() @ q.double().T
    ok = torch.ones_like(s, dtype=torch.bool)
    if tags is not None:
        rs, re, qs = tags
        ok = (re > NOW)[:, None] & ((qs == 0)[None, :] | (rs[:, None] == qs[None, :]))
    out = []
    for b in range(q.shape[0]):
        col, okb = s[:, b].tolist(), ok[:, b].tolist()
        rows = [r for r in range(len(col)) if okb[r]]
        r = max(rows, key=lambda r: (col[r], r), default=-1)
        out.append((r, col[r] if r >= 0 else None))
    return out


@functools.lru_cache(maxsize=None)
def _shape_reference(n_rows, n_q, dim, scoped):
    index, q, *tags = _inputs(n_rows, n_q, dim)
    return _reference(index, q, tags if scoped else None)


def _check(hip, index, q, dtype, tags=None, want=None):
    """Runs the op and compares idx and the decoded scores exactly; returns idx."""
    args = [index.to(dtype).cuda(), q.to(dtype).cuda()]
    if tags is not None:
        args += [t.cuda() for t in tags] + [NOW]
    hi, idx = (t.cpu().tolist() for t in hip.cache_topk_wide(*args))
    want = want or _reference(index, q, tags)
    assert idx == [r for r, _ in want]
    assert [_unorder(h) if r >= 0 else h for h, r in zip(hi, idx)] == \
        [s if r >= 0 else 0 for r, s in want]
    return idx


# 640: 5 chunks, the odd tail of the ping-pong; 2048: the smallest query pass
@pytest.mark.parametrize("dim", [640, 768, 1024, 2048])
@pytest.mark.parametrize("n_q", [1, 17, 129])  # 129: past one pass at every width
@pytest.mark.parametrize("n_rows", [1, 17, N_ROWS])
@DTYPES
def test_shapes(hip, dtype, n_rows, n_q, dim):
    index, q, *tags = _inputs(n_rows, n_q, dim)
    _check(hip, index, q, dtype, want=_shape_reference(n_rows, n_q, dim, False))
    idx = _check(hip, index, q, dtype, tags, _shape_reference(n_rows, n_q, dim, True))
    assert all(i == -1 for i in idx[3::4])  # scope 77 has no row


# the first five: waves 0 and 1 of block 0, block 1, and twice the partial last
# tile (1088..1102); 1100..1102 is its 3-row group
CAND = [40, 300, 1030, 1090, 1101, 3, 41, 130, 260, 515, 700, 1023, 1040, 1088, 1099, 1102]


@pytest.mark.parametrize("dim", [640, 2048])
@DTYPES
def test_every_chunk_counts(hip, dtype, dim):
    """Row CAND[c] is the all-ones query with chunk c zeroed, FULL the query
    itself, every other row zero: dropping, repeating or mis-pairing a chunk
    changes which row wins."""
    cand = CAND[:dim // 128]
    full = 1100
    index = torch.zeros(N_ROWS, dim)
    for c, r in enumerate(cand):
        index[r] = 1.0
        index[r, c * 128:(c + 1) * 128] = 0.0
    index[full] = 1.0
    q = torch.ones(1, dim)
    assert _check(hip, index, q, dtype) == [full]
    expiry = torch.full((N_ROWS,), NOW + 1).int()
    expiry[full] = NOW
    tags = (torch.full((N_ROWS,), 5), expiry, torch.tensor([5]))
    assert _check(hip, index, q, dtype, tags) == [max(cand)]  # all tie: the higher row


@pytest.mark.parametrize("scoped", [False, True])
@DTYPES
def test_tie_inside_one_lanes_rows(hip, dtype, scoped):
    index, q, *_ = (t.clone() for t in _inputs(N_ROWS, 2, 640))
    q[q == 0] = 1.0  # |q|^2 >= dim: well above any random row
    index[40] = index[41] = q[0]
    tags = None
    if scoped:
        tags = (torch.full((N_ROWS,), 5), torch.full((N_ROWS,), NOW + 1).int(),
                torch.tensor([5, 0]))
    assert _check(hip, index, q, dtype, tags)[0] == 41


@pytest.mark.parametrize("dim", [768, 1024])
def test_python_surface(hip, dim):
    cache = SemanticCache(100, dim=dim, capacity=64, device="cuda", _hip=hip,
                          index_dtype="fp8")
    g = torch.Generator().manual_seed(dim)
    v = torch.nn.functional.normalize(torch.randn(5, dim, generator=g), dim=1).cuda()
    slots = [cache.insert(x, b"v") for x in v[:4]]
    found = cache.lookup(v[:4])
    assert [f[0] for f in found] == slots
    assert all(abs(f[1] - 1.0) < 0.02 for f in found)
    slot = cache.insert(v[4], b"scoped", scope=5)
    assert cache.lookup(v[4:], scopes=[9]) == [None]
    assert cache.lookup(v[4:], scopes=[5])[0][0] == slot
    with pytest.raises(ValueError, match="dim <= 512"):
        cache.lookup_k(v[:1], 2)


@pytest.mark.parametrize("dim", [576, 2176])
def test_python_surface_refuses_width(hip, dim):
    with pytest.raises(ValueError, match="multiple of 128"):
        SemanticCache(100, dim=dim, capacity=64, device="cuda", _hip=hip)


def test_services_cache_dim():
    from aigw.gpu import GPUServices

    async def main(text=b"a prompt for the wide cache"):
        gpu = GPUServices(device="cuda", enable_cache=True, cache_dim=768, n_merges=8192,
                          cache_capacity=64)
        try:
            miss, vec = await gpu.cache_lookup_text(text)
            assert miss is None and vec.shape[-1] == 768
            await gpu.cache_insert(vec, b"A")
            assert (await gpu.cache_lookup_text(text))[0] == b"A"
        finally:
            gpu.close()

    asyncio.run(main())
