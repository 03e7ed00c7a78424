"""CPU reference for the semantic cache's MXFP4 index rows (numpy, fp64).

This file is the specification; csrc/mxfp4_kernels.cuh must match it bit
for bit on the packed nibbles and the scale bytes.

A row of ``dim`` values (``dim % 128 == 0``) is stored as OCP MX blocks of
32 elements: one E8M0 scale byte per block and 32 e2m1 nibbles, plus one
fp32 ``inv_norm = 1 / |dequantised row|`` the lookup multiplies in after
the MFMA. The scale is the smallest power of two that does not clip
(``6 * 2^e >= amax``), not the OCP floor rule: docs/TESTING.md has the
accuracy table that decided it.
"""

from __future__ import annotations

import numpy as np

BLOCK = 32
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
# v rounds up past code c's upper midpoint; at the midpoint itself only when
# the code above has the even mantissa bit (codes 1, 3, 5 are the odd ones)
_MID = (E2M1[:-1] + E2M1[1:]) / 2  # .25 .75 1.25 1.75 2.5 3.5 5
_TIE_UP = np.array([False, True, False, True, False, True, False])


def block_exponent(amax: np.ndarray) -> np.ndarray:
    """Smallest integer e with 6 * 2^e >= amax, clamped so that e + 127 is
    in [0, 254]; 0 for amax == 0. Exact: frexp, no logarithm."""
    amax = np.asarray(amax, dtype=np.float64)
    m, ex = np.frexp(amax)  # amax = m * 2^ex, m in [0.5, 1)
    # 6 * 2^e = 0.75 * 2^(e + 3): m <= 0.75 -> e = ex - 3, else ex - 2
    e = np.where(m <= 0.75, ex - 3, ex - 2)
    e = np.where(amax == 0, 0, e)
    return np.clip(e, -127, 127).astype(np.int64)


def round_e2m1(v: np.ndarray) -> np.ndarray:
    """Codes 0..15 (bit 3 = sign) of v rounded to nearest e2m1, ties to the
    even mantissa bit, saturating at +-6. -0 keeps its sign."""
    v = np.asarray(v, dtype=np.float64)
    a = np.abs(v)[..., None]
    code = ((a > _MID) | ((a == _MID) & _TIE_UP)).sum(axis=-1)
    return (code | (np.signbit(v).astype(np.int64) << 3)).astype(np.uint8)


def quantize(x) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """x [n, dim] -> (packed u8 [n, dim/2], scale u8 [n, dim/32],
    inv_norm f32 [n]). Element 2i is the low nibble of byte i (the order
    of torch.float4_e2m1fn_x2)."""
    x = np.asarray(x, dtype=np.float64)
    n, dim = x.shape
    if dim % 128:
        raise ValueError(f"mxfp4: dim must be a multiple of 128, got {dim}")
    xb = x.reshape(n, dim // BLOCK, BLOCK)
    e = block_exponent(np.abs(xb).max(axis=2))
    codes = round_e2m1(xb * np.exp2(-e.astype(np.float64))[..., None]).reshape(n, dim)
    packed = (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)
    scale = (e + 127).astype(np.uint8)
    norm = np.sqrt((dequantize(packed, scale) ** 2).sum(axis=1))
    with np.errstate(divide="ignore"):
        inv_norm = np.where(norm > 0, 1.0 / norm, 0.0).astype(np.float32)
    return packed, scale, inv_norm


def dequantize(packed, scale) -> np.ndarray:
    """fp64 [n, dim] values of packed nibbles and E8M0 scale bytes."""
    packed = np.asarray(packed, dtype=np.uint8)
    scale = np.asarray(scale, dtype=np.uint8)
    n, half = packed.shape
    codes = np.empty((n, half * 2), dtype=np.uint8)
    codes[:, 0::2] = packed & 0xF
    codes[:, 1::2] = packed >> 4
    val = np.where(codes & 8, -1.0, 1.0) * E2M1[codes & 7]
    e = scale.astype(np.float64) - 127
    return (val.reshape(n, -1, BLOCK) * np.exp2(e)[..., None]).reshape(n, half * 2)
