"""MXFP4 index for rows of 640..2048 elements: the slab quantiser bit-exact
against aigw/ops/mxfp4_ref.py, cache_topk_mxfp4_wide against the fp64 product
of the dequantised rows and decoded queries (reference, bound and inputs of
tests/test_gpu_cache_mxfp4.py). Bounds and margins: docs/TESTING.md."""

import asyncio

import numpy as np
import pytest
import torch
from torch.nn.functional import normalize

from aigw.ops import mxfp4_ref as mx
from aigw.ops.semcache import NEVER, SemanticCache, _unorder
from kernel_checks import EPS23
from test_gpu_cache_mxfp4 import NOW, S1, S2, S3, _case, _check, _eligible, _np
from test_gpu_cache_wide import CAND, N_ROWS
from test_mxfp4_ref_cpu import spread_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import aigw_hip

    return aigw_hip


@pytest.mark.parametrize("dim", [640, 1024, 2048])  # 640: a partial second slab; 2048: four
def test_quantizer_bit_exact(hip, dim):
    x = torch.from_numpy(spread_rows(37, dim, dim)).float()
    ties = torch.tensor([6, 2.5, 3.5, .25, .75, 5, 1.25, 1.75, -2.5, -.25, -0.0, -5, -3.5, -.75,
                         4.5, 0.0])
    x[0] = 0.0                                   # all-zero row
    x[1, 32:64] = x[1, 544:576] = 0.0            # all-zero blocks in slabs 0 and 1
    x[2] = ties.repeat(dim // 16) * 8.0          # exact ties, every block at amax 6 * 2^3
    x[3, :32] = x[3, :32].clamp(-20, 20)
    x[3, 512:544] = x[3, 512:544].clamp(-20, 20)
    x[4] = x[3]
    x[3, 5], x[4, 5] = 24.0, -24.125             # amax 6 * 2^2, and the next bf16 above it
    x[3, 517], x[4, 517] = -24.125, 24.0         # the same boundary in slab 1
    x[5, :32] *= 2.0 ** 100                      # huge and tiny blocks in one slab
    x[5, 32:64] *= 2.0 ** -120
    x[6] *= 2.0 ** -120                          # includes bf16 subnormals
    x[7] *= 2.0 ** 100
    x[8, ::3] = -0.0
    x[9, :32] *= 2.0 ** 100                      # huge in slab 0, tiny in the last slab
    x[9, dim - 32:] *= 2.0 ** -120
    x[10, :32] *= 2.0 ** -120                    # and the other way round
    x[10, dim - 32:] *= 2.0 ** 100
    x = x.to(torch.bfloat16)
    assert x[3, 517].item() == -24.125 and x[4, 517].item() == 24.0
    packed, scale, inv_norm = (_np(t) for t in hip.mxfp4_quantize_rows(x.cuda()))
    rp, rs, rn = mx.quantize(x.to(torch.float64).numpy())
    assert (scale == rs).all(), np.argwhere(scale != rs)[:8]
    assert (packed == rp).all(), np.argwhere(packed != rp)[:8]
    assert inv_norm[0] == 0 and rn[0] == 0
    rel = np.abs(inv_norm[1:].astype(np.float64) / rn[1:] - 1)
    print(f"dim {dim}: inv_norm worst rel err {rel.max():.3g}, bound {(dim + 4) * EPS23:.3g}")
    assert (rel <= (dim + 4) * EPS23).all(), rel.argmax()


@pytest.mark.parametrize("n_q", [1, 17, 129])  # 129: past one pass; three passes at 2048
@pytest.mark.parametrize("n_rows", [1, 17, N_ROWS])
@pytest.mark.parametrize("dim", [640, 1024, 2048])
def test_lookup_against_fp64(hip, dim, n_rows, n_q):
    packed, scale, inv_norm, q, w = _case(hip, dim, n_rows, n_q)
    hi, idx = hip.cache_topk_mxfp4_wide(packed, scale, inv_norm, q)
    _check(packed, scale, inv_norm, q, hi, idx, w)
    r = torch.arange(n_rows)  # 3 row scopes, a fifth dead, every 4th query wildcard
    row_scope = torch.tensor([S1, S2, S3])[r % 3]
    row_expiry = torch.where(r % 5 == 2, NOW - (r % 2), NEVER - (r % 2) * (NEVER - NOW - 1))
    row_expiry[w] = NOW + 1
    q_scope = torch.tensor([0 if b % 4 == 0 else (S1, S2, S3)[w[b] % 3] for b in range(n_q)])
    hi, idx = hip.cache_topk_mxfp4_wide(packed, scale, inv_norm, q, row_scope.cuda(),
                                        row_expiry.int().cuda(), q_scope.cuda(), NOW)
    _check(packed, scale, inv_norm, q, hi, idx, w, _eligible(row_scope, row_expiry, q_scope))


@pytest.mark.parametrize("dim", [640, 2048])
def test_every_chunk_counts(hip, dim):
    """Row CAND[c] is the all-ones query with 128-chunk c zeroed, row 1100 the
    query itself, every other row zero (ones are exact in e2m1 and e4m3):
    dropping, repeating or mis-pairing a chunk changes which row wins."""
    cand, full = CAND[:dim // 128], 1100
    index = torch.zeros(N_ROWS, dim)
    for c, r in enumerate(cand):
        index[r] = 1.0
        index[r, c * 128:(c + 1) * 128] = 0.0
    index[full] = 1.0
    rows = hip.mxfp4_quantize_rows(index.to(torch.bfloat16).cuda())
    q = torch.ones(1, dim).to(torch.float8_e4m3fn).cuda()
    hi, idx = hip.cache_topk_mxfp4_wide(*rows, q)
    assert idx.tolist() == [full]
    # an exact integer dot product times inv_norm: its bound and one rounding
    assert abs(_unorder(hi.item()) / dim ** 0.5 - 1) <= (dim + 5) * EPS23
    expiry = torch.full((N_ROWS,), NOW + 1).int()
    expiry[full] = NOW
    hi, idx = hip.cache_topk_mxfp4_wide(*rows, q, torch.full((N_ROWS,), S1).cuda(),
                                        expiry.cuda(), torch.tensor([S1]).cuda(), NOW)
    assert idx.tolist() == [max(cand)]  # all tie: the higher row
    assert abs(_unorder(hi.item()) / (dim - 128) ** 0.5 - 1) <= (dim + 5) * EPS23


@pytest.mark.parametrize("scoped", [False, True])
def test_tie_inside_one_lanes_rows(hip, scoped):
    packed, scale, inv_norm, q, _ = _case(hip, 640, N_ROWS, 2)
    copy = hip.mxfp4_quantize_rows(q[:1].float().to(torch.bfloat16))
    for dst, src in zip((packed, scale, inv_norm), copy):
        dst[40] = dst[41] = src[0]
    tags = ()
    if scoped:
        tags = (torch.full((N_ROWS,), S1).cuda(), torch.full((N_ROWS,), NOW + 1).int().cuda(),
                torch.tensor([S1, 0]).cuda(), NOW)
    assert hip.cache_topk_mxfp4_wide(packed, scale, inv_norm, q, *tags)[1][0].item() == 41


@pytest.mark.parametrize("dim", [768, 1024])
def test_semantic_cache_mxfp4_wide(hip, dim):
    cache = SemanticCache(512, dim=dim, capacity=64, index_dtype="mxfp4", _hip=hip)
    assert cache.index.dtype == torch.uint8 and cache.index.shape == (64, dim // 2)
    vecs = normalize(torch.randn(40, dim, generator=torch.Generator().manual_seed(dim)),
                     dim=1).to(torch.bfloat16).cuda()
    slots = [cache.insert(v, b"r%d" % i) for i, v in enumerate(vecs)]
    hits = cache.lookup(vecs)  # unfiltered
    assert [h and h[0] for h in hits] == slots
    assert all(h[1] >= cache.threshold for h in hits), min(h[1] for h in hits)
    assert [h and h[0] for h in cache.lookup(vecs, scopes=[0] * 40)] == slots  # filtered
    assert cache.lookup(vecs, scopes=[S2] * 40) == [None] * 40  # foreign scope
    with pytest.raises(ValueError, match="mxfp4"):
        cache.lookup_k(vecs[:1], 2)
    assert cache.invalidate() == 40 and cache.lookup(vecs) == [None] * 40


def test_semantic_cache_mxfp4_refuses_width(hip):
    with pytest.raises(ValueError, match="mxfp4"):
        SemanticCache(512, dim=2176, capacity=64, index_dtype="mxfp4", _hip=hip)


def test_services_cache_dim_mxfp4():
    from aigw.gpu import GPUServices

    async def main(text=b"a prompt for the wide mxfp4 cache"):
        gpu = GPUServices(device="cuda", enable_cache=True, cache_dim=768, n_merges=8192,
                          cache_capacity=64, cache_index_dtype="mxfp4")
        try:
            miss, vec = await gpu.cache_lookup_text(text)
            assert miss is None and vec.shape[-1] == 768
            await gpu.cache_insert(vec, b"A")
            assert (await gpu.cache_lookup_text(text))[0] == b"A"
        finally:
            gpu.close()

    asyncio.run(main())
