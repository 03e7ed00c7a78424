"""GPU tests of the prefix-picker kernels: block hashes, the HBM block
index (insert / match / clear_bits) and the scorer with the prefix-hit
term, each held to exact equality with aigw/ops/prefix_ref.py after every
step (cases and comparators in tests/prefix_checks.py, proven sensitive on
the CPU by tests/test_prefix_ref_cpu.py), and one end-to-end pass through
GPUServices.pick_endpoint_prefix."""

import asyncio

import numpy as np
import pytest
import torch

import kernel_checks as kc
import prefix_checks as pc
from aigw.ops import prefix_ref as pr

pytestmark = pytest.mark.gpu

SALT = pr.salt_of("pool-a")


@pytest.fixture(scope="module")
def hip():
    import aigw_hip

    return aigw_hip


def _dev(x, dtype):
    if torch.is_tensor(x):
        return x.to(dtype).cuda().contiguous()
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


# ---- block hashes --------------------------------------------------------------


def _gpu_hashes(hip, ids, off, n, b, mb):
    return hip.prefix_block_hashes(_dev(ids, torch.int32), _dev(off, torch.int64), n,
                                   b, mb, pr.to_i64(SALT))


@pytest.mark.parametrize("max_blocks", [4, 256])
@pytest.mark.parametrize("block_tokens", [8, 16, 64])
@pytest.mark.parametrize("pattern", pc.HASH_PATTERNS)
def test_block_hashes_match_reference(hip, pattern, block_tokens, max_blocks):
    ids, off, n = pc.hash_batch(block_tokens, max_blocks, pattern)
    h, nb = _gpu_hashes(hip, ids, off, n, block_tokens, max_blocks)
    info = pc.check_hashes(h, nb, ids, off, n, block_tokens, max_blocks, SALT)
    assert info["requests"] == 12
    assert info["blocks"] >= 2 * max_blocks  # the two requests at the cap


def test_block_hashes_256_kib_request(hip):
    ids, off, n = pc.big_request_batch()
    h, nb = _gpu_hashes(hip, ids, off, n, 64, 256)
    assert pc.check_hashes(h, nb, ids, off, n, 64, 256, SALT)["blocks"] == 256


def test_block_hashes_ignore_bytes_past_n_bytes_and_empty_input(hip):
    ids, off, n = pc.hash_batch(8, 4, "dense")
    padded = np.concatenate([ids, np.arange(64, dtype=np.int32)])  # stale tail
    h, nb = _gpu_hashes(hip, padded, off, n, 8, 4)
    pc.check_hashes(h, nb, ids, off, n, 8, 4, SALT)
    h, nb = hip.prefix_block_hashes(_dev(ids, torch.int32),
                                    torch.zeros(0, dtype=torch.int64, device="cuda"),
                                    n, 8, 4, 0)
    assert tuple(h.shape) == (0, 4) and tuple(nb.shape) == (0,)


# ---- table -----------------------------------------------------------------------


class GPUBackend:
    def __init__(self, hip, n_buckets, waves=0):
        self.hip, self.waves = hip, waves
        n = n_buckets * pr.SLOTS
        self.keys = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.masks = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.stamps = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.counters = torch.zeros(4, dtype=torch.int32, device="cuda")

    def match(self, hashes, n_blocks, live_mask, now, ttl):
        return self.hip.prefix_match(self.keys, self.masks, self.stamps,
                                     _dev(hashes, torch.int64), _dev(n_blocks, torch.int32),
                                     live_mask, now, ttl)

    def insert(self, hashes, n_blocks, assign, bit_of, now, ttl):
        self.hip.prefix_insert(self.keys, self.masks, self.stamps, self.counters,
                               _dev(hashes, torch.int64), _dev(n_blocks, torch.int32),
                               _dev(assign, torch.int32), _dev(bit_of, torch.int64),
                               now, ttl, waves=self.waves)

    def clear_bits(self, mask):
        self.hip.prefix_clear_bits(self.masks, mask)

    def state(self):
        return self.keys, self.masks, self.stamps, self.counters


_REF_RUNS = {}


def _run_both(hip, table, waves=0):
    steps = pc.table_script(table["batches"], table["max_blocks"])
    key = table["n_buckets"]
    if key not in _REF_RUNS:  # the reference runs once per table
        ref = pc.RefBackend(table["n_buckets"])
        _REF_RUNS[key] = (ref, pc.run_script(ref, steps))
    ref, want = _REF_RUNS[key]
    return ref, want, pc.run_script(GPUBackend(hip, table["n_buckets"], waves), steps)


def test_small_table_with_live_evictions(hip):
    ref, want, got = _run_both(hip, pc.SMALL_TABLE)
    assert ref.t.counters[pr.EVICTED_LIVE] > 0 and ref.t.counters[pr.REUSED_EXPIRED] > 0
    info = pc.check_run(got, want)
    assert info["matches"] > 10


@pytest.mark.parametrize("waves", [0, 8, 1024])
def test_large_table_without_evictions(hip, waves):
    """The table state must not depend on how many waves share the buckets."""
    ref, want, got = _run_both(hip, pc.LARGE_TABLE, waves)
    assert ref.t.counters[pr.EVICTED_LIVE] == 0
    assert np.count_nonzero(ref.t.keys) >= 4000
    pc.check_run(got, want)


def test_table_bindings_reject_bad_inputs_and_skip_empty_ones(hip):
    be = GPUBackend(hip, 4)
    h = torch.zeros(0, 8, dtype=torch.int64, device="cuda")
    nb = torch.zeros(0, dtype=torch.int32, device="cuda")
    assert tuple(be.match(h, nb, -1, 0, 10).shape) == (0, 64)
    be.insert(h, nb, nb, np.array([1], dtype=np.int64), 0, 10)
    assert be.counters.cpu().tolist() == [0, 0, 0, 0]
    one = torch.ones(1, 8, dtype=torch.int64, device="cuda")
    n1 = torch.ones(1, dtype=torch.int32, device="cuda")
    bad_keys = torch.zeros(48, dtype=torch.int64, device="cuda")  # 3 buckets
    with pytest.raises(RuntimeError, match="power of two"):
        hip.prefix_match(bad_keys, bad_keys, bad_keys.int(), one, n1, -1, 0, 10)
    with pytest.raises(RuntimeError, match="int64"):
        hip.prefix_match(be.keys, be.masks, be.stamps, one.int(), n1, -1, 0, 10)
    with pytest.raises(RuntimeError, match="max_blocks"):
        hip.prefix_match(be.keys, be.masks, be.stamps,
                         torch.ones(1, 257, dtype=torch.int64, device="cuda"), n1, -1, 0, 10)
    with pytest.raises(RuntimeError, match="64 replicas"):
        hip.prefix_insert(be.keys, be.masks, be.stamps, be.counters, one, n1,
                          n1, torch.ones(65, dtype=torch.int64, device="cuda"), 0, 10)
    with pytest.raises(RuntimeError, match="block_tokens"):
        hip.prefix_block_hashes(n1, n1.long(), 1, 12, 4, 0)
    with pytest.raises(RuntimeError, match="must be on GPU"):
        hip.prefix_match(be.keys.cpu(), be.masks, be.stamps, one, n1, -1, 0, 10)
    assert int(be.keys.abs().sum()) == 0


# ---- scorer ----------------------------------------------------------------------


def _score(hip, stats, pred, matched, weights, block=pc.SCORE_BLOCK):
    return hip.kv_score_assign_prefix(
        _dev(np.asarray(stats, dtype=np.float32).reshape(-1, 4), torch.float32),
        _dev(np.asarray(pred, dtype=np.float32), torch.float32),
        _dev(matched, torch.int32), block, *weights).cpu().tolist()


@pytest.mark.parametrize("name", sorted(kc.kv_cases()))
def test_zero_weight_and_no_match_equals_kv_score_assign(hip, name):
    stats, pred = kc.kv_cases()[name]
    plain = hip.kv_score_assign(
        torch.tensor(stats, dtype=torch.float32, device="cuda"),
        torch.tensor(pred, dtype=torch.float32, device="cuda"),
        *kc.KV_WEIGHTS).cpu().tolist()
    matched = np.zeros((len(pred), 64), dtype=np.int32)  # the match kernel's stride
    assert _score(hip, stats, pred, matched, kc.KV_WEIGHTS + (0.0,)) == plain
    assert plain == kc.kv_greedy_ref(stats, pred, kc.KV_WEIGHTS, np.float64)


@pytest.mark.parametrize("name", sorted(pc.prefix_kv_cases()))
def test_prefix_scorer_matches_reference(hip, name):
    stats, pred, matched = pc.prefix_kv_cases()[name]
    r32 = pr.score_assign(stats, pred, matched, pc.SCORE_BLOCK, pc.PREFIX_WEIGHTS, np.float32)
    r64 = pr.score_assign(stats, pred, matched, pc.SCORE_BLOCK, pc.PREFIX_WEIGHTS, np.float64)
    assert r32 == r64, "case is not exact in fp32"
    assert _score(hip, stats, pred, matched, pc.PREFIX_WEIGHTS) == r64


# ---- end to end --------------------------------------------------------------------


def _prose(n_words, seed):
    rng = np.random.default_rng(seed)
    words = [b"wave", b"lane", b"cache", b"token", b"prefix", b"block", b"route", b"the",
             b"a", b"of", b"replica", b"gateway", b"scores", b"and", b"holds", b"memory"]
    return b" ".join(words[i] for i in rng.integers(0, len(words), n_words))


def test_pick_endpoint_prefix_end_to_end():
    from aigw.gpu.services import GPUServices

    gpu = GPUServices(device="cuda", n_merges=8192)
    members = ["r0", "r1", "r2", "r3"]
    settings = {"block_tokens": 16, "max_blocks": 256, "buckets": 1024,
                "ttl_s": 300.0, "weight": 1.0}
    equal = [[0.0, 100000.0, 0.0, 0.0]] * 4
    # replica 0 is now the worst row; replica 2 the least loaded
    loaded = [[4000.0, 100000.0, 2.0, 2.0], [100.0, 100000.0, 1.0, 1.0],
              [0.0, 100000.0, 0.0, 0.0], [100.0, 100000.0, 1.0, 1.0]]
    prompt = _prose(250, 1)  # about 800 tokens: some 50 blocks of 16
    follow_up = prompt + b"\n" + _prose(20, 2)
    unrelated = _prose(250, 3)

    async def main():
        first = await gpu.pick_endpoint_prefix("pool", members, equal, prompt, 1024.0,
                                               settings=settings)
        second = await gpu.pick_endpoint_prefix("pool", members, loaded, follow_up,
                                                1024.0, settings=settings)
        third = await gpu.pick_endpoint_prefix("pool", members, loaded, unrelated,
                                               1024.0, settings=settings)
        plain = await gpu.pick_endpoint(loaded, 1024.0)
        return first, second, third, plain

    first, second, third, plain = asyncio.run(main())
    idx = gpu._prefix["pool"]
    # the hashes the service used equal the reference on the tokenizer's ids
    _, ids, state = gpu.tokenizer.encode_batch([prompt], return_ids=True)
    h, nb = idx.hashes(state["out_ids"], state["req_off"], state["n_bytes"])
    want = pr.token_hashes(ids[0], 16, 256, pr.salt_of("pool"))
    n_first = len(want)
    assert 24 <= n_first < 256, "prompt should fill a few dozen blocks"
    assert nb.cpu().tolist() == [n_first]
    assert h.cpu().tolist()[0][:n_first] == [pr.to_i64(x) for x in want]
    assert first.prompt_tokens == len(ids[0])

    assert first == 0 and first.matched_tokens == 0  # a tie on an empty index
    assert plain == 2
    assert second == 0, "the replica holding the conversation wins despite its load"
    # BPE merges stop at the appended text's first byte at the latest, so
    # every block but possibly the last of the first prompt is found again
    assert second.matched_tokens >= (n_first - 1) * 16
    assert third == 2 and third.matched_tokens == 0
    st = idx.stats()
    assert st["members"] == 4 and st["evicted_live"] == 0
    assert st["refreshed"] >= n_first - 1 and st["inserted"] >= 2 * n_first
    gpu.close()
