"""CPU tests of prefix-index replication: the reference semantics
(member_key, refresh_of, PrefixTable.export, apply_remote) on hand-built
tables, the sensitivity of the comparators in tests/prefix_repl_checks.py
to every planted mutant, the config key, and StateSync's prefix collectives
at world 2 on gloo."""

import hashlib
import multiprocessing as mp
import os

import numpy as np
import pytest

import prefix_checks as pc
import prefix_repl_checks as rc
from aigw.filterapi import load_config
from aigw.filterapi.config import ConfigError, PrefixCache
from aigw.ops import prefix_ref as pr

# ---- reference semantics on hand-built tables -------------------------------------

H = 0x1234567890ABCDE1  # bucket 1 of a 4-bucket table
BIT5, BIT63 = 1 << 5, pr.to_i64(1 << 63)


def _table(slot_key=0, mask=0, stamp=0, slot=3):
    t = pr.PrefixTable(4)
    if slot_key:
        s = t.bucket(slot_key) * pr.SLOTS + slot
        t.keys[s], t.masks[s], t.stamps[s] = slot_key, mask, stamp
    return t


def test_member_key_and_refresh_of():
    d = hashlib.sha256(b"replica-a").digest()
    assert pr.member_key("replica-a") == int.from_bytes(d[:8], "little")
    assert pr.member_key(b"replica-a") == pr.member_key("replica-a")
    assert pr.member_key("replica-a") != pr.member_key("replica-b")
    assert 0 < pr.member_key("") < 1 << 64
    assert pr.refresh_of(pr.NEVER) == pr.NEVER
    assert [pr.refresh_of(t) for t in (0, 1, 2, 3, 100, 301)] == [1, 1, 1, 1, 50, 150]


def test_export_rule_on_hand_built_tables():
    ent = [(H, BIT5)]
    ttl, refresh = 100, 50
    assert _table().export(ent, 10, ttl, refresh) == ent  # empty table
    assert _table(H, BIT5, 10).export(ent, 10, ttl, refresh) == []  # bit present, live
    assert _table(H, 1 << 6, 10).export(ent, 10, ttl, refresh) == ent  # key without the bit
    assert _table(H, BIT5, 10).export(ent, 110, ttl, 1000) == ent  # expired slot
    assert _table(H, BIT5, 10).export(ent, 109, ttl, 1000) == []  # its last live second
    assert _table(H, BIT5, 10).export(ent, 10 + refresh - 1, ttl, refresh) == []
    assert _table(H, BIT5, 10).export(ent, 10 + refresh, ttl, refresh) == ent
    # ttl NEVER: never expires and is never re-announced
    never = pr.refresh_of(pr.NEVER)
    assert _table(H, BIT5, 0).export(ent, pr.NEVER - 1, pr.NEVER, never) == []
    # ttl 0: nothing is ever live
    assert _table(H, BIT5, 10).export(ent, 10, 0, pr.refresh_of(0)) == ent
    # bit 63, and a key with bit 63 set (negative as int64)
    neg = pr.to_i64(H | 1 << 63)
    assert _table(neg, BIT63, 10).export([(neg, BIT63)], 10, ttl, refresh) == []
    assert _table(neg, BIT5, 10).export([(neg, BIT63)], 10, ttl, refresh) == [(neg, BIT63)]
    # another key in the same bucket does not count
    assert _table(H + 4, BIT5, 10).export(ent, 10, ttl, refresh) == ent


def test_export_keeps_order_and_duplicates_and_reads_the_table_before_the_list():
    t = _table(H, BIT5, 10)
    ent = [(H + 8, BIT5), (H, BIT5), (H + 4, 1), (H + 8, BIT5), (H, 1)]
    before = (t.keys.copy(), t.masks.copy(), t.stamps.copy())
    assert t.export(ent, 10, 100, 50) == [ent[0], ent[2], ent[3], ent[4]]
    for a, b in zip(before, (t.keys, t.masks, t.stamps)):
        assert (a == b).all(), "export must not change the table"


def test_apply_remote_on_hand_built_tables():
    ka, kb, unknown = (pr.to_i64(pr.member_key(n)) for n in ("a", "b", "zz"))
    t = _table(H, BIT5, 10)
    rec = [(H, ka), (0, ka), (H + 4, unknown), (H + 4, kb), (H, kb), (H, kb)]
    assert pr.apply_remote(t, rec, {ka: 1, kb: BIT63}, 20, 100) == (4, 2)
    s = t.bucket(H) * pr.SLOTS + 3
    assert pr.to_u64(t.masks[s]) == BIT5 | 1 | 1 << 63 and t.stamps[s] == 20
    assert t.block_mask(H + 4, pr.M64, 20, 100) == 1 << 63
    assert t.counters.tolist() == [1, 3, 0, 0]
    # an expired slot is reset, not ORed; keys are compared as uint64
    t = _table(H, BIT5, 10)
    assert pr.apply_remote(t, [(H, pr.to_u64(ka))], {ka: 1}, 110, 100) == (1, 0)
    assert t.masks[s] == 1 and t.counters.tolist() == [0, 1, 1, 0]
    assert pr.apply_remote(pr.PrefixTable(4), [], {}, 0, 100) == (0, 0)


def test_round_trip_between_two_shards_with_different_bits():
    """A inserts, exports and ships; B applies under its own key-to-bit
    map. Each member both know then matches on B as it does on A."""
    rng = np.random.default_rng(3)
    names = ["m%d" % i for i in range(6)]
    a_bit = {n: b for n, b in zip(names, (0, 1, 2, 31, 63, 40))}
    b_bit = {n: b for n, b in zip(names[1:] + ["other"], (63, 0, 7, 32, 1, 9))}
    a, b = pr.PrefixTable(64), pr.PrefixTable(64)
    batches = []
    for now in (10, 20, 30):
        h, nb = pc._keys(rng, 12, 16, 16)
        if batches:
            h[:6, :8] = batches[0][0][:6, :8]  # follow-ups share a prefix
        batches.append((h, nb))
        assign = rng.integers(0, 6, 12)
        bit_of = [1 << a_bit[n] for n in names]
        ent = a.entries(h, nb, assign, bit_of)
        key_by_bit = {pr.to_i64(1 << a_bit[n]): pr.member_key(n) for n in names}
        shipped = [(h_, key_by_bit[bit]) for h_, bit in a.export(ent, now, 100, 50)]
        assert 0 < len(shipped) <= len(ent)
        a.apply(ent, now, 100)
        applied, skipped = pr.apply_remote(
            b, shipped, {pr.member_key(n): 1 << bit for n, bit in b_bit.items()},
            now + 1000, 100)  # B's clock is its own
        assert skipped == sum(1 for _, k in shipped if k == pr.member_key("m0"))
        assert applied + skipped == len(shipped)
    for h, nb in batches:
        ma = a.match(h, nb, pr.M64, 30, 100)
        mb = b.match(h, nb, pr.M64, 1030, 100)
        for n in names[1:]:
            assert (ma[:, a_bit[n]] == mb[:, b_bit[n]]).all(), n
        assert ma[:, a_bit["m1"]].max() > 0
        assert (mb[:, b_bit["other"]] == 0).all()


# ---- the comparators reject every mutant ------------------------------------------


@pytest.fixture(scope="module")
def cases():
    c = dict(rc.export_cases())
    c.update(rc.apply_cases())
    c["walk_small"] = rc.export_walk(pc.SMALL_TABLE)
    return c


@pytest.mark.parametrize("mutant,where", [
    ("refresh_off_by_one", "age_edge"),
    ("ignore_liveness", "dead_under_long_refresh"),
    ("ignore_liveness", "ttl_zero"),
    ("reverse_export", "five_requests"),
    ("reverse_export", "walk_small"),
    ("drop_head", "overflow_mid_request"),
    ("drop_head", "overflow_after_log_n"),
    ("apply_unknown_key", "n_rec_65"),
    ("apply_unknown_key", "one_bucket"),
])
def test_comparator_rejects_mutant(cases, mutant, where):
    assert mutant in rc.REPL_MUTANTS
    assert rc.rejects(cases[where], mutant)


def test_comparator_accepts_the_reference_and_cases_exercise_what_they_claim(cases):
    for name, case in cases.items():
        assert not rc.rejects(case, None), name
    for name in ("walk_small", "five_requests", "twelve_requests", "many_requests",
                 "max_blocks_1", "max_blocks_130", "assign_out_of_range"):
        n_ent, n_exp = rc.export_totals(cases[name])
        assert 0 < n_exp < n_ent, (name, n_ent, n_exp)

    def last(name):
        case = cases[name]
        ref = rc.RefReplBackend(case["n_buckets"], case["cap"], case["log_n"])
        return ref, rc.run_repl_script(ref, case["steps"])[-1]

    _, s = last("overflow_mid_request")
    assert s["repl"].tolist() == [24, 24, 0, 0] and s["log_n"].tolist() == [24]
    _, s = last("log_full")
    assert s["repl"][rc.EXPORTED] == 0 and s["repl"][rc.DROPPED] > 0
    assert (s["log"] == rc.UNTOUCHED).all()
    ref, s = last("one_bucket")
    assert ref.t.counters[pr.EVICTED_LIVE] > 0
    assert s["repl"][rc.APPLIED] > 0 and s["repl"][rc.SKIPPED] > 0
    ref, _ = last("expiring")
    assert ref.t.counters[pr.REUSED_EXPIRED] > 0
    _, s = last("no_members")
    assert s["repl"].tolist() == [0, 0, 0, 65]


# ---- config -------------------------------------------------------------------------


def _cfg(prefix_cache):
    return {"version": "v1", "routes": [{
        "name": "pool", "endpointPicker": True, "prefixCache": prefix_cache,
        "backends": [{"name": "b0", "schema": "OpenAI", "upstream": {"host": "127.0.0.1", "port": 1}}],
    }]}


def test_prefix_cache_replicate_key():
    assert PrefixCache().replicate is False
    assert load_config(_cfg({})).routes[0].prefix_cache.replicate is False
    assert load_config(_cfg({"replicate": True})).routes[0].prefix_cache.replicate is True
    assert load_config(_cfg({"replicate": False, "ttlS": 5})).routes[0].prefix_cache == \
        PrefixCache(ttl_s=5)
    # what the server hands GPUServices: unchanged unless the key is on
    assert PrefixCache().settings() == {"block_tokens": 16, "max_blocks": 256,
                                        "buckets": 65536, "ttl_s": 300.0, "weight": 1.0}
    assert PrefixCache(replicate=True).settings()["replicate"] is True
    for bad in (1, 0, "true", None, [True]):
        with pytest.raises(ConfigError, match="replicate"):
            load_config(_cfg({"replicate": bad}))


# ---- StateSync at world 2 on gloo ---------------------------------------------------


class FakePrefix:
    """Records what StateSync hands it (GPUServices' two blocking calls)."""

    def __init__(self):
        import torch

        self.pending = torch.zeros(0, 3, dtype=torch.int64)
        self.applied = []
        self.asked = []

    def add(self, rows):
        import torch

        self.pending = torch.cat([self.pending, rows])

    def prefix_drain_sync(self, max_n):
        self.asked.append(max_n)
        out, self.pending = self.pending[:max_n], self.pending[max_n:]
        return out

    def prefix_apply_sync(self, rows):
        assert rows.dtype.is_floating_point is False and rows.shape[1] == 3
        self.applied.append(rows.clone())


class FakeCache:
    dim = 8

    def __init__(self):
        self.pending, self.remote = [], []

    def drain_pending(self, max_n=32):
        import torch

        batch, self.pending = self.pending[:max_n], self.pending[max_n:]
        if not batch:
            return torch.zeros(0, self.dim, dtype=torch.bfloat16), []
        return torch.stack([v for v, _ in batch]).to(torch.bfloat16), [r for _, r in batch]

    def insert_remote(self, vec, value):
        self.remote.append(value)


def _rows(rank, lo, n):
    """n distinct rows that tell their rank and position."""
    import torch

    i = torch.arange(lo, lo + n, dtype=torch.int64)
    return torch.stack([i + 1, torch.full_like(i, -(rank + 1)), i * 7 - 3], dim=1)


def _sync_worker(rank: int, world: int, port: int, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch
        import torch.distributed as dist

        from aigw.filterapi.config import RateLimitRule
        from aigw.parallel import StateSync
        from aigw.ratelimit import RateLimiter

        dist.init_process_group("gloo", rank=rank, world_size=world)
        calls = {"all_gather": 0, "all_reduce": 0}
        real_gather, real_reduce = dist.all_gather, dist.all_reduce

        def gather(*a, **k):
            calls["all_gather"] += 1
            return real_gather(*a, **k)

        def reduce(*a, **k):
            calls["all_reduce"] += 1
            return real_reduce(*a, **k)

        dist.all_gather, dist.all_reduce = gather, reduce

        def tick(sync):
            before = dict(calls)
            sync.tick_sync()
            return (calls["all_reduce"] - before["all_reduce"],
                    calls["all_gather"] - before["all_gather"])

        limiter = RateLimiter(
            [RateLimitRule(name="b", metadata_key="llm_total_token", limit=10, window_s=60)])
        other = 1 - rank
        # no prefix at all: a tick is today's single all-reduce
        assert tick(StateSync(limiter)) == (1, 0)

        fake = FakePrefix()
        sync = StateSync(limiter, prefix=fake)
        cap = sync.MAX_PREFIX_RECORDS_PER_TICK
        assert cap == 16384
        # nothing to send anywhere: the count all-gather only
        assert tick(sync) == (1, 1) and fake.applied == [] and fake.asked == [cap]
        # one rank with zero records
        if rank == 0:
            fake.add(_rows(0, 0, 3))
        assert tick(sync) == (1, 2)
        if rank == 1:
            assert len(fake.applied) == 1 and torch.equal(fake.applied[0], _rows(0, 0, 3))
        else:
            assert fake.applied == []
        # both ranks, different counts: only the other rank's rows, unpadded
        fake.applied.clear()
        fake.add(_rows(rank, 10, 5 if rank == 0 else 2))
        assert tick(sync) == (1, 2)
        assert len(fake.applied) == 1
        assert torch.equal(fake.applied[0], _rows(other, 10, 2 if rank == 0 else 5))
        # more than the per-tick cap: the remainder follows on the next tick
        fake.applied.clear()
        if rank == 1:
            fake.add(_rows(1, 100, cap + 10))
        assert tick(sync) == (1, 2) and tick(sync) == (1, 2) and tick(sync) == (1, 1)
        if rank == 0:
            assert [a.shape[0] for a in fake.applied] == [cap, 10]
            assert torch.equal(torch.cat(fake.applied), _rows(1, 100, cap + 10))
        else:
            assert fake.applied == [] and fake.pending.shape[0] == 0
        # cache sync in the same tick
        fake.applied.clear()
        cache = FakeCache()
        both = StateSync(limiter, cache, fake)
        if rank == 0:
            cache.pending.append((torch.ones(8), b"answer"))
        fake.add(_rows(rank, 500, 4))
        assert tick(both) == (1, 3 + 2)  # cache: sizes, rows, payload; prefix: count, block
        assert torch.equal(fake.applied[0], _rows(other, 500, 4))
        assert cache.remote == ([b"answer"] if rank == 1 else [])
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback

        q.put((rank, f"FAIL: {e}\n{traceback.format_exc()}"))


def test_state_sync_prefix_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sync_worker, args=(r, 2, 29793, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=30)
        if p.is_alive():
            p.terminate()
            pytest.fail("worker hung")
    for rank, status in results:
        assert status == "ok", f"rank {rank}: {status}"
