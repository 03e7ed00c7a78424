"""CPU tests of the prefix-picker reference (aigw/ops/prefix_ref.py) and of
the comparators in tests/prefix_checks.py that the GPU tests rely on."""

import numpy as np
import pytest

import kernel_checks as kc
import prefix_checks as pc
from aigw.ops import prefix_ref as pr

SALT = pr.salt_of("pool-a")


def _tokens(n, seed=0):
    return np.random.default_rng(seed).integers(0, pc.VOCAB, n)


# ---- reference properties ----------------------------------------------------


def test_extending_a_prompt_keeps_its_earlier_hashes():
    t = _tokens(200)
    short = pr.token_hashes(t[:100], 16, 256, SALT)
    long = pr.token_hashes(t, 16, 256, SALT)
    assert len(short) == 6 and len(long) == 12
    assert long[:6] == short


def test_swapping_two_tokens_changes_that_hash_and_every_later_one():
    t = _tokens(160, 1)
    u = t.copy()
    assert u[35] != u[36]
    u[35], u[36] = u[36], u[35]  # inside block 2
    a, b = pr.token_hashes(t, 16, 256, SALT), pr.token_hashes(u, 16, 256, SALT)
    assert a[:2] == b[:2]
    assert all(x != y for x, y in zip(a[2:], b[2:])) and len(a) == 10


def test_a_different_salt_changes_every_hash():
    t = _tokens(256, 2)
    a = pr.token_hashes(t, 16, 256, SALT)
    b = pr.token_hashes(t, 16, 256, pr.salt_of("pool-b"))
    assert len(a) == 16 and all(x != y for x, y in zip(a, b))


def test_random_prompts_give_distinct_nonzero_keys():
    keys = set()
    for i in range(256):
        keys.update(pr.token_hashes(_tokens(256, 100 + i), 16, 256, SALT))
    assert len(keys) == 4096 and 0 not in keys


def test_only_full_blocks_count_and_max_blocks_caps():
    t = _tokens(100, 3)
    assert len(pr.token_hashes(t, 8, 256, SALT)) == 12
    assert len(pr.token_hashes(t, 8, 4, SALT)) == 4
    assert pr.token_hashes(t[:7], 8, 4, SALT) == []
    # past max_blocks the tokens do not matter
    assert pr.token_hashes(t[:40], 8, 4, SALT) == pr.token_hashes(t, 8, 4, SALT)


def test_zero_hash_is_remapped():
    assert pr.chain([0], 0) == [1]  # mix(0) == 0: key 0 means "empty slot"


def _one(h, bit=1):
    return [(pr.to_i64(h), bit)]


def test_ttl_edge():
    t = pr.PrefixTable(4)
    t.apply(_one(77), now=10, ttl=100)
    h, nb = np.array([[77]], dtype=np.int64), np.array([1], dtype=np.int32)
    assert t.match(h, nb, pr.M64, 109, 100)[0, 0] == 1  # now - stamp == ttl - 1
    assert t.match(h, nb, pr.M64, 110, 100)[0, 0] == 0  # now - stamp == ttl
    assert t.match(h, nb, pr.M64, 10 ** 9, pr.NEVER)[0, 0] == 1


def test_reinserting_an_expired_key_resets_its_mask():
    t = pr.PrefixTable(4)
    t.apply(_one(77, 1), 10, 100)
    t.apply(_one(77, 2), 20, 100)
    slot = int(np.nonzero(t.keys == 77)[0][0])
    assert t.masks[slot] == 3 and t.stamps[slot] == 20
    t.apply(_one(77, 4), 120, 100)  # 120 - 20 == ttl: expired
    assert t.masks[slot] == 4 and t.stamps[slot] == 120
    assert t.counters.tolist() == [1, 2, 1, 0]


def test_victim_order_is_empty_then_expired_then_oldest():
    t = pr.PrefixTable(1)
    for i in range(16):  # fill the bucket; slot i has stamp 10 + i
        t.apply(_one(100 + i), 10 + i, 100)
    assert t.keys.tolist() == list(range(100, 116))
    t.keys[5] = 0  # an empty slot wins over everything
    t.apply(_one(200), 30, 100)
    assert t.keys[5] == 200
    # slots 0 (stamp 10) and 1 (stamp 11) are expired at now 111: lowest first
    t.apply(_one(201), 111, 100)
    assert t.keys[0] == 201 and t.counters[pr.REUSED_EXPIRED] == 1
    # ttl NEVER: nothing is expired, the smallest stamp (slot 1) goes
    t.apply(_one(202), 112, pr.NEVER)
    assert t.keys[1] == 202 and t.counters[pr.EVICTED_LIVE] == 1
    # ties on the stamp: lowest index
    t.stamps[:] = 50
    t.apply(_one(203), 113, pr.NEVER)
    assert t.keys[0] == 203


def test_match_run_breaks_at_a_missing_block_and_bit63_counts():
    t = pr.PrefixTable(8)
    bit63 = pr.to_i64(1 << 63)
    t.apply([(11, bit63), (12, bit63), (14, bit63)], 0, 100)
    h = np.array([[11, 12, 13, 14]], dtype=np.int64)
    m = t.match(h, np.array([4], dtype=np.int32), pr.M64, 0, 100)
    assert m[0, 63] == 2 and m[0].sum() == 2
    t.clear_bits(bit63)
    assert t.match(h, np.array([4], dtype=np.int32), pr.M64, 0, 100).sum() == 0


# ---- comparator sensitivity --------------------------------------------------

HASH_CASE = (8, 4)  # block_tokens, max_blocks: small, every token count covered


@pytest.mark.parametrize("pattern", pc.HASH_PATTERNS)
def test_hash_comparator_accepts_the_correct_emulation(pattern):
    b, mb = HASH_CASE
    ids, off, n = pc.hash_batch(b, mb, pattern)
    h, nb = pc.emulate_hashes(ids, off, n, b, mb, SALT)
    info = pc.check_hashes(h, nb, ids, off, n, b, mb, SALT)
    assert info["requests"] == 12 and info["blocks"] > 20


def test_hash_comparator_accepts_the_big_request():
    ids, off, n = pc.big_request_batch()
    h, nb = pc.emulate_hashes(ids, off, n, 64, 256, SALT)
    assert pc.check_hashes(h, nb, ids, off, n, 64, 256, SALT)["blocks"] == 256
    assert nb.tolist() == [256, 0]


@pytest.mark.parametrize("mutant", pc.HASH_MUTANTS)
@pytest.mark.parametrize("pattern", pc.HASH_PATTERNS)
def test_hash_comparator_rejects_wrong_emulations(pattern, mutant):
    b, mb = HASH_CASE
    ids, off, n = pc.hash_batch(b, mb, pattern)
    h, nb = pc.emulate_hashes(ids, off, n, b, mb, SALT, mutant=mutant)
    with pytest.raises(AssertionError):
        pc.check_hashes(h, nb, ids, off, n, b, mb, SALT)


@pytest.fixture(scope="module")
def small_run():
    steps = pc.table_script(pc.SMALL_TABLE["batches"], pc.SMALL_TABLE["max_blocks"])
    ref = pc.RefBackend(pc.SMALL_TABLE["n_buckets"])
    return steps, pc.run_script(ref, steps), ref


def test_small_table_script_evicts_live_entries(small_run):
    steps, want, ref = small_run
    assert ref.t.counters[pr.EVICTED_LIVE] > 0
    assert ref.t.counters[pr.REUSED_EXPIRED] > 0
    again = pc.run_script(pc.RefBackend(pc.SMALL_TABLE["n_buckets"]), steps)
    info = pc.check_run(again, want)
    assert info["matches"] > 10
    # the script sees hits, broken runs and bit 63
    assert any(s.get("matched") is not None and s["matched"][:, 63].max() > 0 for s in want)


@pytest.mark.parametrize("mutant", pc.TABLE_MUTANTS)
def test_table_comparator_rejects_wrong_emulations(small_run, mutant):
    steps, want, _ = small_run
    got = pc.run_script(pc.RefBackend(pc.SMALL_TABLE["n_buckets"], mutant=mutant), steps)
    with pytest.raises(AssertionError):
        pc.check_run(got, want)


def test_large_table_script_evicts_nothing():
    steps = pc.table_script(pc.LARGE_TABLE["batches"], pc.LARGE_TABLE["max_blocks"])
    ref = pc.RefBackend(pc.LARGE_TABLE["n_buckets"])
    for s in steps:
        if s["op"] == "insert":
            ref.insert(s["hashes"], s["n_blocks"], s["assign"], s["bit_of"],
                       s["now"], s["ttl"])
    assert ref.t.counters[pr.EVICTED_LIVE] == 0
    assert np.count_nonzero(ref.t.keys) >= 4000


# ---- scorer ------------------------------------------------------------------


@pytest.mark.parametrize("name", sorted(pc.prefix_kv_cases()))
def test_prefix_kv_cases_are_exact_in_fp32(name):
    stats, pred, matched = pc.prefix_kv_cases()[name]
    r32 = pr.score_assign(stats, pred, matched, pc.SCORE_BLOCK, pc.PREFIX_WEIGHTS, np.float32)
    r64 = pr.score_assign(stats, pred, matched, pc.SCORE_BLOCK, pc.PREFIX_WEIGHTS, np.float64)
    assert r32 == r64


def test_affinity_and_load_cases_say_what_they_claim():
    cases = pc.prefix_kv_cases()

    def run(name, w_p=1.0):
        stats, pred, matched = cases[name]
        w = pc.PREFIX_WEIGHTS[:3] + (w_p,)
        return pr.score_assign(stats, pred, matched, pc.SCORE_BLOCK, w, np.float64)

    assert run("affinity_over_load") == [2] and run("affinity_over_load", 0.0) != [2]
    assert run("load_over_affinity") == [0]
    # capped at p: the hit term is exactly w_p and the nearly full replica is
    # charged nothing, so it fits and wins once (1 + 2^-9 against 1 - 2^-8);
    # its queued request then costs it more than the idle replica's KV term
    assert run("hit_over_p") == [3, 0]
    # the prefix term changes assignments in the mixed cases
    stats, pred, matched = cases["mixed_64"]
    plain = kc.kv_greedy_ref(stats, pred, kc.KV_WEIGHTS, np.float64)
    assert run("mixed_64") != plain


@pytest.mark.parametrize("name", sorted(kc.kv_cases()))
def test_zero_weight_and_no_match_is_the_plain_scorer(name):
    stats, pred = kc.kv_cases()[name]
    matched = np.zeros((len(pred), len(stats)), dtype=np.int32)
    got = pr.score_assign(stats, pred, matched, 16, kc.KV_WEIGHTS + (0.0,), np.float32)
    assert got == kc.kv_greedy_ref(stats, pred, kc.KV_WEIGHTS, np.float32)
