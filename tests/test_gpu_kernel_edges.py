"""GPU kernel edge tests: every HIP kernel at the shapes where kernels go
wrong (partial tiles, K tails, block and wave boundaries, empty inputs),
held to exact rows / exact ids or to a-priori floating-point error bounds
against fp64 CPU references (comparators in tests/kernel_checks.py, proven
sensitive on the CPU by tests/test_kernel_checks_cpu.py)."""

import numpy as np
import pytest
import torch

import kernel_checks as kc

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float8_e4m3fn]
DTYPE_IDS = ["bf16", "fp8"]


@pytest.fixture(scope="module")
def hip():
    import aigw_hip

    return aigw_hip


def _topk(hip, index, q):
    hi, idx = hip.cache_topk(index.cuda().contiguous(), q.cuda().contiguous())
    return hi.cpu(), idx.cpu()


def _quant(x: torch.Tensor, dtype) -> torch.Tensor:
    return x.to(torch.bfloat16).to(dtype)


# ---------------------------------------------------------------------------
# cache_topk
# ---------------------------------------------------------------------------

N_ROWS = 1100  # a full 1024-row block + a block whose first wave ends in a 12-row tile


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_topk_every_row_position_wins_once(hip, dtype):
    """Planted-winner sweep, dim 384: in 5 calls of <= 256 queries every
    row 0..1099 is the exact argmax of exactly one query, so a row lost by
    the tile masking, the ping-pong buffers, the cross-lane or LDS folds,
    or the second pass's offset is a wrong answer, not a near miss."""
    index = kc.unit_rows(N_ROWS, 384, dtype, seed=384)
    worst = 0.0
    for lo in range(0, N_ROWS, 256):
        winners = list(range(lo, min(lo + 256, N_ROWS)))
        q = index[torch.tensor(winners)].clone()
        hi, idx = _topk(hip, index, q)
        stats = kc.check_topk(hi, idx, index, q)
        assert idx.tolist() == winners
        assert stats["min_gap"] > 0.5
        worst = max(worst, stats["max_err_over_bound"])
    print(f"topk sweep {dtype}: max |err|/bound = {worst:.3f}")


STRUCTURAL = [0, 15, 16, 255, 256, 1023, 1024, 1088, 1099]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("dim", [128, 256, 512])
def test_topk_structural_winners_other_dims(hip, dim, dtype):
    index, q = kc.planted_case(N_ROWS, dim, dtype, STRUCTURAL, seed=dim)
    hi, idx = _topk(hip, index, q)
    stats = kc.check_topk(hi, idx, index, q)
    assert idx.tolist() == STRUCTURAL
    print(f"topk dim {dim} {dtype}: {stats}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n_q", [1, 129])
def test_topk_row_count_edges(hip, n_q, dtype):
    """Index sizes around the 16-row tile, the 256-row wave span and the
    1024-row block; winners at row 0 and at the last row."""
    for n_rows in (1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025):
        for first in (0, n_rows - 1):
            # alternate so a 129-query call has both winners in both passes
            winners = [first if b % 2 == 0 else n_rows - 1 - first
                       for b in range(n_q)]
            index, q = kc.planted_case(n_rows, 384, dtype, winners,
                                       seed=7000 + n_rows)
            hi, idx = _topk(hip, index, q)
            kc.check_topk(hi, idx, index, q)
            assert idx.tolist() == winners, (n_rows, first)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_topk_all_negative_scores(hip, dtype):
    """Every index row is anti-correlated with every query: the least
    negative row must come back exactly (the orderable-float transform's
    negative branch, and -1e30 masking that must stay below real scores)."""
    g = torch.Generator().manual_seed(31)
    dim = 384
    u = torch.nn.functional.normalize(torch.randn(dim, generator=g), dim=0)
    for winner in (0, 300, 1099):
        w = torch.nn.functional.normalize(torch.randn(N_ROWS, dim, generator=g), dim=1)
        c = 1.0 + 2.0 * torch.rand(N_ROWS, generator=g)
        c[winner] = 0.3
        index = _quant(-torch.nn.functional.normalize(c[:, None] * u + w, dim=1), dtype)
        noise = torch.randn(17, dim, generator=g) / dim ** 0.5
        q = _quant(torch.nn.functional.normalize(u + 0.1 * noise, dim=1), dtype)
        assert float((index.double() @ q.double().T).max()) < -0.1
        hi, idx = _topk(hip, index, q)
        stats = kc.check_topk(hi, idx, index, q)
        assert idx.tolist() == [winner] * 17
        assert stats["min_gap"] > 0.1


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_topk_zero_rows(hip, dtype):
    """All-zero index except one planted row that is the NEGATED query 0:
    query 0 must get a zero row (any of them) with score exactly 0.0. The
    other queries' expected winners come from the fp64 scores: the planted
    row where it scores positive, a zero row where it scores negative."""
    from aigw.ops.semcache import _unorder

    g = torch.Generator().manual_seed(41)
    dim = 384
    for planted in (0, 500, 1099):
        q0 = torch.nn.functional.normalize(torch.randn(dim, generator=g), dim=0)
        signs = torch.tensor([1.0, -1.0, 1.0, -1.0, -1.0, 1.0])
        noise = torch.nn.functional.normalize(torch.randn(6, dim, generator=g), dim=1)
        others = torch.nn.functional.normalize(signs[:, None] * q0 + noise, dim=1)
        q = _quant(torch.cat([q0[None], others]), dtype)
        index_f = torch.zeros(N_ROWS, dim)
        index_f[planted] = -q[0].float()
        index = _quant(index_f, dtype)
        S = index.double() @ q.double().T
        zero_rows = set(range(N_ROWS)) - {planted}
        allowed = [None if float(S[planted, b]) > 0 else zero_rows
                   for b in range(q.shape[0])]
        assert allowed[0] is zero_rows and float(S[planted, 0]) < -0.9
        assert any(a is None for a in allowed) and sum(a is not None for a in allowed) >= 3
        hi, idx = _topk(hip, index, q)
        kc.check_topk(hi, idx, index, q, allowed_rows=allowed)
        assert _unorder(int(hi[0])) == 0.0 and int(idx[0]) != planted


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_topk_exact_ties(hip, dtype):
    """The same row planted twice. Which copy wins is unspecified (lowest
    row within a lane's 4 rows, highest across lanes/waves/blocks); either
    is accepted, the score must still be exact."""
    pairs = [(36, 38),     # same tile, same lane group (rows 36..39)
             (10, 300),    # waves 0 and 1 of block 0
             (100, 1050)]  # blocks 0 and 1
    index_f = kc.unit_rows(N_ROWS, 384, dtype, seed=51).float()
    for a, b in pairs:
        index_f[b] = index_f[a]
    index = _quant(index_f, dtype)
    q = index[torch.tensor([a for a, _ in pairs])].clone()
    hi, idx = _topk(hip, index, q)
    kc.check_topk(hi, idx, index, q, allowed_rows=[set(p) for p in pairs])


# ---------------------------------------------------------------------------
# gemm_bf16_nt
# ---------------------------------------------------------------------------

def _gemm_case(hip, m, n, k, with_bias, relu, seed):
    a, bt, bias = kc.gemm_inputs(m, n, k, seed, with_bias)
    c = hip.gemm_bf16_nt(a.cuda(), bt.cuda(),
                         bias.cuda() if bias is not None else None, relu)
    stats = kc.check_gemm(c, a, bt, bias, relu)
    print(f"gemm {(m, n, k)} bias={with_bias} relu={relu}: {stats}")


@pytest.mark.parametrize("m,n,k", [(1, 1, 8), (16, 64, 8), (17, 65, 24),
                                   (33, 100, 40), (5, 130, 200), (250, 70, 72)])
def test_gemm_simple_path_k_tails(hip, m, n, k):
    """K % 32 != 0 reaches the per-lane kk < K tail; M and N off the 16x64
    tile reach the row/column guards."""
    _gemm_case(hip, m, n, k, False, False, seed=m * 1000 + k)
    _gemm_case(hip, m, n, k, True, True, seed=m * 1000 + k + 1)


@pytest.mark.parametrize("m,n,k,combos", [
    (128, 128, 32, [(True, True), (True, False), (False, True)]),
    (256, 384, 96, [(True, True), (True, False), (False, True)]),
    (1024, 128, 64, [(True, True)]),  # 8 workgroups: swizzle branch, r == 0
])
def test_gemm_tiled_path_bias_relu(hip, m, n, k, combos):
    for i, (with_bias, relu) in enumerate(combos):
        _gemm_case(hip, m, n, k, with_bias, relu, seed=m + n + k + i)


# ---------------------------------------------------------------------------
# kv_score_assign
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(kc.kv_cases()))
def test_kv_score_assign_exact_cases(hip, name):
    stats, pred = kc.kv_cases()[name]
    r32 = kc.kv_greedy_ref(stats, pred, kc.KV_WEIGHTS, np.float32)
    r64 = kc.kv_greedy_ref(stats, pred, kc.KV_WEIGHTS, np.float64)
    assert r32 == r64, "case is not exact in fp32"
    got = hip.kv_score_assign(
        torch.tensor(stats, dtype=torch.float32, device="cuda"),
        torch.tensor(pred, dtype=torch.float32, device="cuda"),
        *kc.KV_WEIGHTS).cpu().tolist()
    assert got == r64


# ---------------------------------------------------------------------------
# l2norm_rows
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [32, 100, 384, 1000])
def test_l2norm_rows_scales_and_zero_row(hip, dim):
    g = torch.Generator().manual_seed(dim)
    for rows in (1, 4, 5, 37):
        x = torch.randn(rows, dim, generator=g)
        x *= torch.logspace(-3, 3, rows)[:, None] if rows > 1 else 1e3
        zero = rows // 2 if rows > 1 else None
        if zero is not None:
            x[zero] = 0
        out = hip.l2norm_rows(x.cuda()).cpu()
        assert out.dtype == torch.bfloat16 and out.shape == x.shape
        x64 = x.double()
        norm = x64.norm(dim=1, keepdim=True)
        ref = torch.where(norm > 0, x64 / norm.clamp_min(1e-300), torch.zeros_like(x64))
        # one bf16 rounding (2^-9) plus the fp32 norm error, together < 2^-8
        tol = 2.0 ** -8 * ref.abs() + 1e-30
        err = (out.double() - ref).abs()
        assert torch.isfinite(out.float()).all()
        assert (err <= tol).all(), (rows, float((err / tol).max()))
        if zero is not None:
            assert torch.equal(out[zero].float(), torch.zeros(dim))
    z = hip.l2norm_rows(torch.zeros(1, dim, device="cuda")).cpu().float()
    assert torch.equal(z, torch.zeros(1, dim))


# ---------------------------------------------------------------------------
# meanpool
# ---------------------------------------------------------------------------

def _meanpool_layout():
    """Synthetic (ids, req_off): -1 holes, a single-token request, an
    EMPTY request in the middle, a 1000-token request (all 8 position
    blocks contribute), and a short tail request."""
    rng = np.random.default_rng(61)
    vocab = 500

    def req(n_tok, n_pos):
        ids = np.full(n_pos, -1, dtype=np.int32)
        pos = np.sort(rng.choice(n_pos, n_tok, replace=False))
        ids[pos] = rng.integers(0, vocab, n_tok)
        return ids

    reqs = [req(25, 50), req(1, 3), np.zeros(0, np.int32), req(1000, 1400), req(7, 9)]
    offs = np.cumsum([0] + [len(r) for r in reqs[:-1]]).astype(np.int64)
    return np.concatenate(reqs), offs, reqs, vocab


@pytest.mark.parametrize("dim", [2, 100, 384, 1024])
def test_meanpool_synthetic_ids(hip, dim):
    ids, offs, reqs, vocab = _meanpool_layout()
    g = torch.Generator().manual_seed(dim)
    emb = torch.randn(vocab, dim, generator=g).to(torch.bfloat16)
    out = hip.meanpool(torch.from_numpy(ids).cuda(), torch.from_numpy(offs).cuda(),
                       emb.cuda()).cpu()
    assert out.shape == (len(reqs), dim)
    emb64 = emb.double()
    for r, rid in enumerate(reqs):
        toks = torch.from_numpy(rid[rid >= 0].astype(np.int64))
        cnt = toks.numel()
        if cnt == 0:
            assert torch.equal(out[r], torch.zeros(dim)), "empty request row"
            continue
        rows = emb64[toks]
        ref = rows.mean(dim=0)
        bound = (cnt + 2) * kc.EPS23 * rows.abs().mean(dim=0)
        err = (out[r].double() - ref).abs()
        assert (err <= bound).all(), (r, cnt, float((err / bound.clamp_min(1e-300)).max()))


# ---------------------------------------------------------------------------
# BPE
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tok(hip):
    from aigw.ops.tokenizer import GPUTokenizer

    return GPUTokenizer(n_merges=8192, device="cuda")


@pytest.fixture(scope="module")
def bpe_ref(tok):
    return tok.reference()


def _check_bpe(tok, bpe_ref, texts):
    """bpe_encode and bpe_count_async against BPERef.encode_batch: ids and
    counts identical to the oracle, hence to each other."""
    expect = bpe_ref.encode_batch(texts)
    counts, ids, _ = tok.encode_batch(texts, return_ids=True)
    assert ids == expect, _first_diff(ids, expect, texts)
    assert counts.cpu().tolist() == [len(e) for e in expect]
    counts_a, out_ids, _off, ev = tok.encode_batch_async(texts)
    ev.synchronize()
    assert counts_a.cpu().tolist() == [len(e) for e in expect]
    flat = out_ids.cpu().numpy()
    bounds = np.cumsum([0] + [len(t) for t in texts])
    ids_a = [[int(x) for x in flat[bounds[i]:bounds[i + 1]] if x >= 0]
             for i in range(len(texts))]
    assert ids_a == expect, _first_diff(ids_a, expect, texts)


def _first_diff(got, want, texts):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"request {i} (len {len(texts[i])}): got {g[:12]} want {w[:12]}"
    return "length mismatch"


BPE_CASES = kc.bpe_cases()


@pytest.mark.parametrize("name", sorted(BPE_CASES))
def test_bpe_edges_match_reference(tok, bpe_ref, name):
    texts = BPE_CASES[name]
    _check_bpe(tok, bpe_ref, texts)
    if name.startswith("empty"):
        counts, ids, _ = tok.encode_batch(texts, return_ids=True)
        for t, c, i in zip(texts, counts.cpu().tolist(), ids):
            if not t:
                assert c == 0 and i == []
