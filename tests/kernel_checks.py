"""Comparators and input builders for the HIP kernel edge tests.

Plain helper module (no tests here): tests/test_kernel_checks_cpu.py proves
on the CPU that each comparator rejects deliberately wrong emulations, and
tests/test_gpu_kernel_edges.py feeds them the real kernels' outputs.

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
    from aigw.ops.semcache import _unorder

    hi = _as_list(hi)
    idx = _as_list(idx)
    index64 = index.detach().cpu().to(torch.float64)
    q64 = q.detach().cpu().to(torch.float64)
    n_rows, dim = index64.shape
    n_q = q64.shape[0]
    assert len(hi) == n_q and len(idx) == n_q, (len(hi), len(idx), n_q)
    S = index64 @ q64.T  # (N, B), exact up to fp64 rounding
    row_norm = index64.norm(dim=1)
    q_norm = q64.norm(dim=1)
    max_row_norm = float(row_norm.max())
    worst_err, worst_ratio, min_gap = 0.0, 0.0, float("inf")
    for b in range(n_q):
        col = S[:, b]
        smax = float(col.max())
        if allowed_rows is not None and allowed_rows[b] is not None:
            allowed = sorted(int(r) for r in allowed_rows[b])
            for r in allowed:
                assert float(col[r]) == smax, (
                    f"query {b}: allowed row {r} scores {float(col[r])!r}, "
                    f"not the exact maximum {smax!r}")
        else:
            allowed = [int(col.argmax())]
        # fitness of the inputs: best row outside the allowed set
        if len(allowed) < n_rows:
            rest = col.clone()
            rest[allowed] = -float("inf")
            gap = smax - float(rest.max())
            gap_tol = dim * EPS23 * max_row_norm * float(q_norm[b])
            assert gap > 100.0 * gap_tol, (
                f"query {b}: inputs unfit for an exact-row check, top-1/top-2 "
                f"gap {gap:.3e} <= 100 x {gap_tol:.3e}")
            min_gap = min(min_gap, gap)
        row = int(idx[b])
        assert 0 <= row < n_rows, f"query {b}: row {row} out of range"
        assert row in allowed, (
            f"query {b}: got row {row} (exact score {float(col[row]):.6f}), "
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
            "min_gap": min_gap}


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
