"""MXFP4 cache index on the GPU: the quantiser bit-exact against
aigw/ops/mxfp4_ref.py, the scaled-MFMA lookup against the fp64 product of the
dequantised rows and decoded queries. Bounds and margins: docs/TESTING.md."""

import numpy as np
import pytest
import torch
from torch.nn.functional import normalize

from aigw.ops import mxfp4_ref as mx
from aigw.ops.semcache import NEVER, SemanticCache, _unorder
from kernel_checks import EPS23
from test_mxfp4_ref_cpu import spread_rows

pytestmark = pytest.mark.gpu

NOW = 1000
S1, S2, S3 = 0x1111111111, -0x2222222222, 0x3333333333


@pytest.fixture(scope="module")
def hip():
    import aigw_hip

    return aigw_hip


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("dim", [128, 384, 512])
def test_quantizer_bit_exact(hip, dim):
    x = torch.from_numpy(spread_rows(37, dim, dim)).float()
    ties = torch.tensor([6, 2.5, 3.5, .25, .75, 5, 1.25, 1.75, -2.5, -.25, -0.0, -5, -3.5, -.75,
                         4.5, 0.0])
    x[0] = 0.0                                   # all-zero row
    x[1, 32:64] = 0.0                            # one all-zero block
    x[2] = ties.repeat(dim // 16) * 8.0          # exact ties, every block at amax 6 * 2^3
    x[3, :32] = x[3, :32].clamp(-20, 20)
    x[4] = x[3]
    x[3, 5], x[4, 5] = 24.0, -24.125             # amax 6 * 2^2, and the next bf16 above it
    x[5, :32] *= 2.0 ** 100                      # huge and tiny blocks in one row
    x[5, 32:64] *= 2.0 ** -120
    x[6] *= 2.0 ** -120                          # includes bf16 subnormals
    x[7] *= 2.0 ** 100
    x[8, ::3] = -0.0
    x = x.to(torch.bfloat16)
    assert x[3, 5].item() == 24.0 and x[4, 5].item() == -24.125
    packed, scale, inv_norm = (_np(t) for t in hip.mxfp4_quantize_rows(x.cuda()))
    rp, rs, rn = mx.quantize(x.to(torch.float64).numpy())
    assert (scale == rs).all(), np.argwhere(scale != rs)[:8]
    assert (packed == rp).all(), np.argwhere(packed != rp)[:8]
    assert inv_norm[0] == 0 and rn[0] == 0
    rel = np.abs(inv_norm[1:].astype(np.float64) / rn[1:] - 1)
    print(f"dim {dim}: inv_norm worst rel err {rel.max():.3g}, bound {(dim + 4) * EPS23:.3g}")
    assert (rel <= (dim + 4) * EPS23).all(), rel.argmax()


def _case(hip, dim, n_rows, n_q, winners=None):
    """Per query b a planted winner: q[b] = normalize(row w[b] + 0.5 * unit noise)."""
    gen = torch.Generator().manual_seed(dim * 7 + n_rows * 3 + n_q)
    rows = normalize(torch.from_numpy(spread_rows(n_rows, dim, dim + n_rows)).float(), dim=1)
    packed, scale, inv_norm = hip.mxfp4_quantize_rows(rows.to(torch.bfloat16).cuda())
    w = winners or [(b * 37 + 5) % n_rows for b in range(n_q)]
    unit = normalize(torch.from_numpy(mx.dequantize(_np(packed), _np(scale))[w]).float(), dim=1)
    noise = normalize(torch.randn(n_q, dim, generator=gen), dim=1)
    q = normalize(unit + 0.5 * noise, dim=1).to(torch.float8_e4m3fn)
    return packed, scale, inv_norm, q.cuda(), w


def _eligible(row_scope, row_expiry, q_scope):
    return ((row_expiry > NOW)[:, None]
            & ((q_scope == 0)[None, :] | (row_scope[:, None] == q_scope[None, :]))).numpy()


def _check(packed, scale, inv_norm, q, hi, idx, want, elig=None):
    """Reference: deq @ q.T * inv_norm in fp64, -inf where ineligible; bound:
    dim * 2^-23 * sum|a||b| * inv_norm + 2^-23 * |score| of the winning row."""
    deq, qd = mx.dequantize(_np(packed), _np(scale)), _np(q.float()).astype(np.float64)
    inv = _np(inv_norm)[:, None].astype(np.float64)
    score = deq @ qd.T * inv
    bound = deq.shape[1] * EPS23 * (np.abs(deq) @ np.abs(qd).T * inv) + EPS23 * np.abs(score)
    if elig is not None:
        score = np.where(elig, score, -np.inf)
    assert score.argmax(axis=0).tolist() == want
    if len(deq) > 1:  # from the reference alone: gaps clear 100x the worst row's bound
        top2 = np.sort(score, axis=0)[-2:]
        assert ((top2[1] - top2[0]) >= 100 * bound.max(axis=0)).all(), "reference gap too small"
    assert idx.cpu().tolist() == want
    cols = np.arange(len(want))
    ratio = np.abs(np.array([_unorder(h) for h in hi.cpu().tolist()]) - score[want, cols])
    ratio /= bound[want, cols]
    print(f"dim {deq.shape[1]}: worst |err| / bound {ratio.max():.4f}")
    assert (ratio <= 1).all(), ratio.max()


@pytest.mark.parametrize("n_q", [1, 16, 17, 129, 256])
@pytest.mark.parametrize("n_rows", [1, 15, 17, 1103])
@pytest.mark.parametrize("dim", [128, 384, 512])
def test_lookup_against_fp64(hip, dim, n_rows, n_q):
    packed, scale, inv_norm, q, w = _case(hip, dim, n_rows, n_q)
    hi, idx = hip.cache_topk_mxfp4(packed, scale, inv_norm, q)
    _check(packed, scale, inv_norm, q, hi, idx, w)
    r = torch.arange(n_rows)  # 3 row scopes, a fifth dead, every 4th query wildcard
    row_scope = torch.tensor([S1, S2, S3])[r % 3]
    row_expiry = torch.where(r % 5 == 2, NOW - (r % 2), NEVER - (r % 2) * (NEVER - NOW - 1))
    row_expiry[w] = NOW + 1
    q_scope = torch.tensor([0 if b % 4 == 0 else (S1, S2, S3)[w[b] % 3] for b in range(n_q)])
    hi, idx = hip.cache_topk_mxfp4_scoped(packed, scale, inv_norm, q, row_scope.cuda(),
                                          row_expiry.int().cuda(), q_scope.cuda(), NOW)
    _check(packed, scale, inv_norm, q, hi, idx, w, _eligible(row_scope, row_expiry, q_scope))


def test_mask_hides_better_ineligible_rows(hip):
    """Row w ^ 1 copies the query but is foreign, expiry == now, or expired under
    a wildcard query; slack rows past n_rows hold eligible copies of query 0."""
    dim, n_rows, n_q, slack = 384, 1103, 129, 64
    w = [8 * b + 2 * (b % 4) for b in range(n_q - 2)] + [1100, 1090]
    packed, scale, inv_norm, q, _ = _case(hip, dim, n_rows + slack, n_q, w)
    copies = hip.mxfp4_quantize_rows(q.float().to(torch.bfloat16))
    row_scope = torch.full((n_rows + slack,), S1)
    row_expiry = torch.full((n_rows + slack,), NEVER)
    q_scope = torch.full((n_q,), S1)
    q_scope[2::3] = 0
    q_scope[-1] = S3
    decoy = torch.tensor(w[:-1]) ^ 1
    row_scope[decoy[0::3]] = S2
    row_expiry[decoy[1::3]] = NOW
    row_expiry[decoy[2::3]] = NOW - 5
    for dst, src in zip((packed, scale, inv_norm), copies):
        dst[decoy.cuda()] = src[:-1]
        dst[n_rows:] = src[0]
    view = [t[:n_rows] for t in (packed, scale, inv_norm)]
    hi, idx = hip.cache_topk_mxfp4(*view, q[:-1])  # unmasked, the copies win
    _check(*view, q[:-1], hi, idx, decoy.tolist())
    row_scope, row_expiry = row_scope[:n_rows], row_expiry[:n_rows]
    hi, idx = hip.cache_topk_mxfp4_scoped(*view, q, row_scope.cuda(), row_expiry.int().cuda(),
                                          q_scope.cuda(), NOW)
    elig = _eligible(row_scope, row_expiry, q_scope)
    assert not elig[:, -1].any() and idx[-1].item() == -1 and hi[-1].item() == 0
    _check(*view, q[:-1], hi[:-1], idx[:-1], w[:-1], elig[:, :-1])


def test_semantic_cache_mxfp4(hip):
    with pytest.raises(ValueError, match="mxfp4"):
        SemanticCache(512, dim=192, capacity=64, index_dtype="mxfp4", _hip=hip)
    cache = SemanticCache(512, dim=384, capacity=64, index_dtype="mxfp4", _hip=hip)
    assert cache.index.dtype == torch.uint8 and cache.index.shape == (64, 192)
    vecs = normalize(torch.randn(40, 384, generator=torch.Generator().manual_seed(40)),
                     dim=1).to(torch.bfloat16).cuda()
    slots = [cache.insert(v, b"r%d" % i) for i, v in enumerate(vecs)]
    hits = cache.lookup(vecs)  # unfiltered kernel
    assert [h and h[0] for h in hits] == slots
    assert all(h[1] >= cache.threshold for h in hits), min(h[1] for h in hits)
    assert [h and h[0] for h in cache.lookup(vecs, scopes=[0] * 40)] == slots  # filtered
    assert cache.lookup(vecs, scopes=[S2] * 40) == [None] * 40  # foreign scope
    assert cache.invalidate() == 40 and cache.lookup(vecs) == [None] * 40
