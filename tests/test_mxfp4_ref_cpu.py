"""aigw/ops/mxfp4_ref.py, the specification of the MXFP4 index format."""

import numpy as np
import pytest
import torch

from aigw.ops import mxfp4_ref as mx


def _bf16(x):
    return torch.as_tensor(x, dtype=torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def spread_rows(n, dim, seed):
    """bf16 rows whose 32-blocks differ in magnitude by 2^k, k in -3..3."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, dim // 32, 32)) * np.exp2(g.integers(-3, 4, (n, dim // 32, 1)))
    return _bf16(x.reshape(n, dim))


@pytest.mark.parametrize("dim", [128, 384])
def test_round_trip(dim):
    x = spread_rows(37, dim, dim)
    x[0] = 0.0
    x[1, 32:64] = 0.0
    packed, scale, inv_norm = mx.quantize(x)
    d = mx.dequantize(packed, scale)
    # idempotent in value: an amax rounded down to 3 * 2^e takes scale e - 1 next time
    p2, s2, n2 = mx.quantize(d)
    assert (mx.dequantize(p2, s2) == d).all() and (n2 == inv_norm).all()
    # no element clips, and the scale is the smallest that does not
    limit = 6.0 * np.exp2(scale.astype(np.float64) - 127)
    amax = np.abs(x.reshape(37, -1, 32)).max(axis=2)
    assert (amax <= limit).all() and ((amax > limit / 2) | (amax == 0)).all()
    assert (scale[0] == 127).all() and (packed[0] == 0).all() and inv_norm[0] == 0
    assert scale[1, 1] == 127 and (packed[1, 16:32] == 0).all()
    np.testing.assert_allclose(inv_norm[1:], 1 / np.linalg.norm(d[1:], axis=1), rtol=2**-23)


def test_ties_sign_and_packing():
    x = np.zeros((1, 128))
    # amax 6 -> e = 0, so the values below are rounded as written
    x[0, :12] = [6, 2.5, 3.5, 0.25, 0.75, 5, -2.5, -0.25, 1.25, 1.75, -0.0, -5]
    packed, scale, _ = mx.quantize(x)
    got = mx.dequantize(packed, scale)[0, :12]
    want = np.array([6, 2, 4, 0, 1, 4, -2, -0.0, 1, 2, -0.0, -4])
    assert (got == want).all() and (np.signbit(got) == np.signbit(want)).all()
    # element 2i in the low nibble: (6, 2) -> 7 | 4 << 4, (-0, -4) -> 8 | 14 << 4
    assert scale[0, 0] == 127 and packed[0, 0] == 0x47 and packed[0, 5] == 0xE8


@pytest.mark.parametrize("k", [-130, -127, -3, 0, 5, 100, 125])
def test_scale_boundary(k):
    at = 6.0 * 2.0**k  # 1.5 * 2^(k+2): a bf16 ulp there is 2^(k-5), 2^-133 if subnormal
    above = at + 2.0 ** max(k - 5, -133)
    assert _bf16(at) == at and _bf16(above) == above  # neighbours in bf16
    x = np.zeros((2, 128))
    x[0, 7], x[1, 7] = at, -above
    _, scale, _ = mx.quantize(x)
    assert scale[0, 0] == min(max(k + 127, 0), 254) and scale[1, 0] == min(max(k + 128, 0), 254)


def _floor_rule(x):
    """OCP MX scale: e = floor(log2 amax) - 2, elements saturate at 6."""
    xb = x.reshape(x.shape[0], -1, 32)
    _, ex = np.frexp(np.abs(xb).max(axis=2))
    s = np.exp2(ex - 1.0 - 2.0)[..., None]
    c = mx.round_e2m1(xb / s)
    return ((np.where(c & 8, -1.0, 1.0) * mx.E2M1[c & 7]) * s).reshape(x.shape)


def test_score_error_ordering():
    """4000 bf16 unit-vector pairs, dim 384, cosine 0.92; error against their product."""
    g = np.random.default_rng(384)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    a = unit(g.standard_normal((4000, 384)))
    n = g.standard_normal((4000, 384))
    n = unit(n - (n * a).sum(1, keepdims=True) * a)
    a, b = _bf16(a), _bf16(0.92 * a + np.sqrt(1 - 0.92**2) * n)
    fp8 = lambda v: torch.as_tensor(v, dtype=torch.float32).to(torch.float8_e4m3fn).to(
        torch.float64).numpy()
    packed, scale, inv_norm = mx.quantize(a)
    ours = mx.dequantize(packed, scale)
    rows = {
        "fp8 x fp8": (fp8(a) * fp8(b)).sum(1),
        "mxfp4 x mxfp4, floor rule": (_floor_rule(a) * _floor_rule(b)).sum(1),
        "mxfp4 x fp8, floor rule": (_floor_rule(a) * fp8(b)).sum(1),
        "mxfp4 x fp8, non-clipping": (ours * fp8(b)).sum(1),
        "mxfp4 x fp8, non-clipping, inv_norm": (ours * fp8(b)).sum(1) * inv_norm,
    }
    err = {name: score - (a * b).sum(1) for name, score in rows.items()}
    for name, e in err.items():
        print(f"{name:38s} mean {e.mean():+.4f} std {e.std():.4f} max {np.abs(e).max():.4f}")
    assert err["mxfp4 x fp8, non-clipping, inv_norm"].std() < err["mxfp4 x fp8, floor rule"].std()
