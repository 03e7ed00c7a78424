"""GPU tests of prefix-index replication: prefix_export and
prefix_apply_remote held to exact equality with aigw/ops/prefix_ref.py
after every step (table, table counters, the whole log, log_n and the
replication counters; cases and comparator in tests/prefix_repl_checks.py,
proven sensitive on the CPU by tests/test_prefix_repl_cpu.py), the
bindings' input checks, and one end-to-end pass through two PrefixIndex
objects of one pool."""

import numpy as np
import pytest
import torch

import prefix_checks as pc
import prefix_repl_checks as rc
from aigw.ops import prefix_ref as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import aigw_hip

    return aigw_hip


def _dev(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


class GPUReplBackend:
    def __init__(self, hip, n_buckets, cap, log_n=0, waves=0):
        self.hip, self.waves = hip, waves
        n = n_buckets * pr.SLOTS
        self.keys = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.masks = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.stamps = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.counters = torch.zeros(4, dtype=torch.int32, device="cuda")
        self.log = torch.full((cap, 2), rc.UNTOUCHED, dtype=torch.int64, device="cuda")
        self.log_n = torch.full((1,), log_n, dtype=torch.int32, device="cuda")
        self.repl = torch.zeros(4, dtype=torch.int32, device="cuda")

    def insert(self, hashes, n_blocks, assign, bit_of, now, ttl):
        self.hip.prefix_insert(self.keys, self.masks, self.stamps, self.counters,
                               _dev(hashes, torch.int64), _dev(n_blocks, torch.int32),
                               _dev(assign, torch.int32), _dev(bit_of, torch.int64),
                               now, ttl)

    def clear_bits(self, mask):
        self.hip.prefix_clear_bits(self.masks, mask)

    def export(self, hashes, n_blocks, assign, bit_of, key_of, now, ttl, refresh):
        self.hip.prefix_export(self.keys, self.masks, self.stamps,
                               _dev(hashes, torch.int64), _dev(n_blocks, torch.int32),
                               _dev(assign, torch.int32), _dev(bit_of, torch.int64),
                               _dev(key_of, torch.int64), self.log, self.log_n, self.repl,
                               now, ttl, refresh)

    def apply_remote(self, rec, member_keys, member_bits, now, ttl):
        rec = _dev(np.asarray(rec, dtype=np.int64).reshape(-1, 2), torch.int64)
        self.hip.prefix_apply_remote(self.keys, self.masks, self.stamps, self.counters,
                                     rec, rec.shape[0], _dev(member_keys, torch.int64),
                                     _dev(member_bits, torch.int64), self.repl, now, ttl,
                                     waves=self.waves)

    def state(self):
        return self.keys, self.masks, self.stamps, self.counters

    def repl_state(self):
        return self.log, self.log_n, self.repl


_WANT = {}


def _check(hip, name, case, waves=0):
    if name not in _WANT:  # the reference runs once per case
        ref = rc.RefReplBackend(case["n_buckets"], case["cap"], case["log_n"])
        _WANT[name] = (ref, rc.run_repl_script(ref, case["steps"]))
    ref, want = _WANT[name]
    gpu = GPUReplBackend(hip, case["n_buckets"], case["cap"], case["log_n"], waves)
    rc.check_repl_run(rc.run_repl_script(gpu, case["steps"]), want)
    return ref, want


# ---- export ----------------------------------------------------------------------


@pytest.mark.parametrize("table", ["SMALL_TABLE", "LARGE_TABLE"])
def test_export_rides_the_table_scripts(hip, table):
    case = rc.export_walk(getattr(pc, table))
    # accepted only if the reference exports some entries and not all
    n_ent, n_exp = rc.export_totals(case)
    assert 0 < n_exp < n_ent, (n_ent, n_exp)
    assert sum(s["op"] == "insert" for s in case["steps"]) >= 6
    _check(hip, table, case)


_EXPORT_CASES = rc.export_cases()


@pytest.mark.parametrize("name", sorted(_EXPORT_CASES))
def test_export_shapes_and_rule_edges(hip, name):
    _, want = _check(hip, name, _EXPORT_CASES[name])
    last = want[-1]
    if name == "overflow_mid_request":
        assert last["repl"].tolist() == [24, 24, 0, 0]
    if name in ("log_full", "overflow_after_log_n"):
        assert last["repl"][rc.DROPPED] > 0
    if name == "zero_requests":
        assert last["log_n"].tolist() == [0]


# ---- apply_remote ----------------------------------------------------------------

_APPLY_CASES = rc.apply_cases()


@pytest.mark.parametrize("name", sorted(_APPLY_CASES))
def test_apply_remote_matches_reference(hip, name):
    ref, want = _check(hip, name, _APPLY_CASES[name])
    if name == "one_bucket":
        assert ref.t.counters[pr.EVICTED_LIVE] > 0
    if name.startswith("n_rec_"):
        n = int(name.split("_")[-1])
        assert want[-1]["repl"][rc.APPLIED] + want[-1]["repl"][rc.SKIPPED] == n


@pytest.mark.parametrize("waves", [0, 8, 1024])
@pytest.mark.parametrize("name", ["large", "one_bucket"])
def test_apply_remote_does_not_depend_on_waves(hip, name, waves):
    _check(hip, name, _APPLY_CASES[name], waves)


# ---- bindings --------------------------------------------------------------------


def test_bindings_reject_bad_inputs_and_leave_the_table_untouched(hip):
    be = GPUReplBackend(hip, 4, 16)
    one = torch.ones(1, 8, dtype=torch.int64, device="cuda")
    n1 = torch.ones(1, dtype=torch.int32, device="cuda")
    a0 = torch.zeros(1, dtype=torch.int32, device="cuda")
    b1 = torch.ones(1, dtype=torch.int64, device="cuda")
    b65 = torch.ones(65, dtype=torch.int64, device="cuda")
    bad_keys = torch.zeros(48, dtype=torch.int64, device="cuda")  # 3 buckets
    rec = torch.ones(3, 2, dtype=torch.int64, device="cuda")

    def export(keys=be.keys, masks=be.masks, stamps=be.stamps, hashes=one, n_blocks=n1,
               assign=a0, bit_of=b1, key_of=b1, log=be.log, log_n=be.log_n, repl=be.repl,
               now=0, ttl=10, refresh=5):
        hip.prefix_export(keys, masks, stamps, hashes, n_blocks, assign, bit_of, key_of,
                          log, log_n, repl, now, ttl, refresh)

    def apply(keys=be.keys, masks=be.masks, stamps=be.stamps, counters=be.counters,
              rec=rec, n_rec=3, mk=b1, mb=b1, repl=be.repl, now=0, ttl=10, waves=0):
        hip.prefix_apply_remote(keys, masks, stamps, counters, rec, n_rec, mk, mb, repl,
                                now, ttl, waves=waves)

    for call, kw, msg in [
        (export, dict(keys=bad_keys, masks=bad_keys, stamps=bad_keys.int()), "power of two"),
        (export, dict(hashes=one.int()), "int64"),
        (export, dict(assign=a0.long()), "assign must be int32"),
        (export, dict(bit_of=b65, key_of=b65), "64 replicas"),
        (export, dict(key_of=torch.ones(2, dtype=torch.int64, device="cuda")), "key_of"),
        (export, dict(log=be.log.reshape(-1)), r"log must be int64\[cap, 2\]"),
        (export, dict(log=be.log.int()), r"log must be int64\[cap, 2\]"),
        (export, dict(log_n=be.log_n.long()), r"log_n must be int32\[1\]"),
        (export, dict(repl=be.counters[:3]), r"repl_counters must be int32\[4\]"),
        (export, dict(refresh=-1), "non-negative int32"),
        (export, dict(log=be.log.cpu()), "must be on GPU"),
        (apply, dict(keys=bad_keys, masks=bad_keys, stamps=bad_keys.int()), "power of two"),
        (apply, dict(rec=rec.int()), r"rec must be int64\[n, 2\]"),
        (apply, dict(rec=torch.ones(3, 3, dtype=torch.int64, device="cuda")),
         r"rec must be int64\[n, 2\]"),
        (apply, dict(n_rec=4), "n_rec"),
        (apply, dict(n_rec=-1), "n_rec"),
        (apply, dict(mk=b65, mb=b65), "64 replicas"),
        (apply, dict(mb=torch.ones(2, dtype=torch.int64, device="cuda")), "member_bits"),
        (apply, dict(mk=b1.int()), "member_keys must be int64"),
        (apply, dict(repl=be.repl.long()), r"repl_counters must be int32\[4\]"),
        (apply, dict(waves=5000), "waves"),
        (apply, dict(rec=rec.cpu()), "must be on GPU"),
    ]:
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    assert int(be.keys.abs().sum()) == 0 and int(be.masks.abs().sum()) == 0
    assert be.log_n.item() == 0 and be.repl.tolist() == [0, 0, 0, 0]
    assert bool((be.log == rc.UNTOUCHED).all())
    # n_rec below rec.size(0) applies the first n_rec records only
    apply(n_rec=0)
    assert be.repl.tolist() == [0, 0, 0, 0]
    apply(n_rec=2, mk=torch.full((1,), 1, dtype=torch.int64, device="cuda"))
    assert be.repl.tolist() == [0, 0, 2, 0] and be.counters.tolist() == [1, 1, 0, 0]


# ---- end to end ------------------------------------------------------------------


def _prose(n_words, seed):
    rng = np.random.default_rng(seed)
    words = [b"wave", b"lane", b"cache", b"token", b"prefix", b"block", b"route", b"the",
             b"a", b"of", b"replica", b"gateway", b"scores", b"and", b"holds", b"memory"]
    return b" ".join(words[i] for i in rng.integers(0, len(words), n_words))


def test_follow_up_on_another_shard_finds_its_prefix():
    from aigw.gpu.services import GPUServices
    from aigw.ops.prefixindex import PrefixIndex

    gpu = GPUServices(device="cuda", n_merges=8192)  # does the tokenising
    hip = gpu.tokenizer.hip
    members = ["r0", "r1", "r2", "r3"]
    kw = dict(block_tokens=16, max_blocks=256, buckets=1024, ttl_s=300.0, _hip=hip)

    def index(order, replicate=True):
        idx = PrefixIndex("pool", replicate=replicate, **kw)
        idx.set_members(order)  # bits in this shard's own order
        return idx

    a, b, b_alone = index(members), index(members[::-1]), index(members[::-1])
    off = index(members, replicate=False)
    assert a.set_members(members) != b.set_members(members)

    def pick(idx, text, rows):
        counts, out_ids, req_off, _ev = gpu.tokenizer.encode_batch_async([text])
        stats = torch.tensor(rows, dtype=torch.float32, device="cuda")
        pred = torch.tensor([1024.0], dtype=torch.float32, device="cuda")
        assign, hit, nb = idx.assign(members, stats, pred, out_ids, req_off, len(text))
        return int(assign[0]), int(hit[0]) * idx.block_tokens, int(nb[0])

    # replica 1 is a little ahead at first; afterwards it is the worst row
    # and replica 2 the least loaded
    first_rows = [[100.0, 100000.0, 1.0, 1.0], [0.0, 100000.0, 0.0, 0.0],
                  [100.0, 100000.0, 1.0, 1.0], [100.0, 100000.0, 1.0, 1.0]]
    loaded = [[100.0, 100000.0, 1.0, 1.0], [4000.0, 100000.0, 2.0, 2.0],
              [0.0, 100000.0, 0.0, 0.0], [100.0, 100000.0, 1.0, 1.0]]
    prompt = _prose(250, 1)  # about 800 tokens: some 50 blocks of 16
    follow_up = prompt + b"\n" + _prose(20, 2)

    chosen, matched, n_first = pick(a, prompt, first_rows)
    assert chosen == 1 and matched == 0 and 24 <= n_first < 256
    assert pick(off, prompt, first_rows)[0] == 1
    assert off.stats()["exported"] == 0 and off.log is None
    st = a.stats()
    assert st["exported"] == n_first and st["dropped"] == 0 and st["inserted"] == n_first

    rec = a.drain_log(16384)
    assert tuple(rec.shape) == (n_first, 2) and rec.dtype == torch.int64 and rec.is_cuda
    assert rec[:, 1].tolist() == [pr.to_i64(pr.member_key("r1"))] * n_first
    assert a.drain_log(16384).shape[0] == 0  # drained
    b.apply_remote(rec)
    assert b.stats()["applied"] == n_first and b.stats()["skipped"] == 0

    # B: the replica A chose wins despite its load; without the apply step
    # the least-loaded one does
    chosen_b, matched_b, _ = pick(b, follow_up, loaded)
    assert chosen_b == 1
    assert matched_b >= (n_first - 1) * 16
    assert pick(b_alone, follow_up, loaded)[:2] == (2, 0)
    # the same prompt again on A goes to the same replica: nothing new to say
    a_before = a.stats()["exported"]
    pick(a, prompt, loaded)
    assert a.stats()["exported"] == a_before
    gpu.close()


def test_gpu_services_drain_and_apply_route_rows_by_salt():
    import asyncio

    from aigw.gpu.services import GPUServices

    gpu = GPUServices(device="cuda", n_merges=8192)
    s = dict(block_tokens=16, max_blocks=64, buckets=256, ttl_s=300.0, weight=1.0,
             replicate=True)
    gpu.prefix_prepare("pool-a", s)
    gpu.prefix_prepare("pool-b", s)
    gpu.prefix_prepare("pool-c", dict(s, replicate=False))
    assert sorted(gpu._prefix) == ["pool-a", "pool-b", "pool-c"]
    assert gpu._prefix["pool-a"].replicate and not gpu._prefix["pool-c"].replicate
    assert tuple(gpu.prefix_drain_sync(16384).shape) == (0, 3)
    members = ["r0", "r1"]
    rows4 = [[0.0, 100000.0, 0.0, 0.0]] * 2
    picks = asyncio.run(gpu.assign_replicas_prefix(
        "pool-a", members, rows4, [_prose(120, 4), _prose(120, 5)], None, s))
    n = sum(p.prompt_tokens // 16 for p in picks)
    assert n >= 20
    head = gpu.prefix_drain_sync(5)
    rows = torch.cat([head, gpu.prefix_drain_sync(16384)])
    assert tuple(head.shape) == (5, 3) and tuple(rows.shape) == (n, 3) and rows.is_cuda
    assert set(rows[:, 2].tolist()) == {pr.to_i64(pr.salt_of("pool-a"))}
    assert set(rows[:, 1].tolist()) <= {pr.to_i64(pr.member_key(m)) for m in members}
    # as another shard would receive them: for pool-b, for a pool that does
    # not replicate here, and for one that is not built here
    gpu._prefix["pool-b"].set_members(members[::-1])
    mixed = rows.cpu().repeat(3, 1)
    for i, pool in enumerate(["pool-b", "pool-c", "nowhere"]):
        mixed[i::3, 2] = pr.to_i64(pr.salt_of(pool))
    gpu.prefix_apply_sync(mixed)
    assert gpu.prefix_rows_dropped == 2 * n
    st = gpu.prefix_stats()
    assert st["pool-b"]["applied"] == n and st["pool-b"]["inserted"] == n
    assert st["pool-c"]["applied"] == 0 and st["pool-a"]["applied"] == 0
    assert st["pool-a"]["exported"] == n
    gpu.close()


def test_drain_log_keeps_the_remainder_in_order(hip):
    from aigw.ops.prefixindex import PrefixIndex

    idx = PrefixIndex("pool", buckets=64, replicate=True, _hip=hip)
    h, nb = pc._keys(np.random.default_rng(9), 3, 16, 16)
    bits = idx.set_members(["x", "y"])
    assign = torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")
    idx.export(_dev(h, torch.int64), _dev(nb, torch.int32), assign, ["x", "y"], bits, now=0)
    want = [[int(h[r, k]), pr.to_i64(pr.member_key("xyx"[r]))]
            for r in range(3) for k in range(16)]
    got = idx.drain_log(10).tolist() + idx.drain_log(0).tolist() + idx.drain_log(30).tolist()
    assert int(idx.log_n.item()) == 8
    got += idx.drain_log(100).tolist()
    assert got == want and idx.drain_log(5).shape[0] == 0
