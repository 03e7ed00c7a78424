"""Cases, backends and comparators for prefix-index replication.

As tests/prefix_checks.py does for the picker kernels: one scripted
scenario runs against the reference (aigw.ops.prefix_ref), a deliberately
wrong emulation of it (a "mutant") or the HIP kernels, and the comparator
demands exact equality with the reference after every step: the table, its
counters, the whole replication log (untouched rows included), log_n and
the four replication counters. tests/test_prefix_repl_cpu.py shows on the
CPU that the comparator rejects every mutant on these very cases.
"""

from __future__ import annotations

import numpy as np

import prefix_checks as pc
from aigw.ops import prefix_ref as pr

REPL_MUTANTS = ("refresh_off_by_one", "ignore_liveness", "reverse_export", "drop_head",
                "apply_unknown_key")
EXPORTED, DROPPED, APPLIED, SKIPPED = range(4)
MEMBERS = ("r0", "r1", "r2", "r3")  # stats rows 0..3 hold pc.REPLICA_BITS
REFRESH = pr.refresh_of(pc.TTL)
UNTOUCHED = -7  # what a log row holds before anything is written to it
WALK_CAP = 65536


def keys_of(names) -> np.ndarray:
    return np.array([pr.to_i64(pr.member_key(n)) for n in names], dtype=np.int64)


def bits_of(bits) -> np.ndarray:
    return np.array([pr.to_i64(1 << b) for b in bits], dtype=np.int64)


def log_append(log: np.ndarray, log_n: int, rows, mutant=None):
    """The log's semantics: rows are appended at log_n in order; when fewer
    than all fit, the first ones that fit are kept. Returns (log_n, kept,
    dropped)."""
    room = max(len(log) - log_n, 0)
    kept = rows[:room]
    if mutant == "drop_head" and len(rows) > room:
        kept = rows[len(rows) - room:]
    for i, row in enumerate(kept):
        log[log_n + i] = row
    return log_n + len(kept), len(kept), len(rows) - len(kept)


class RefReplBackend(pc.RefBackend):
    """prefix_ref behind the backend interface of the scripts below,
    optionally with one of REPL_MUTANTS planted."""

    def __init__(self, n_buckets: int, cap: int, log_n: int = 0, mutant=None):
        super().__init__(n_buckets)
        self.repl_mutant = mutant
        self.log = np.full((cap, 2), UNTOUCHED, dtype=np.int64)
        self.log_n = log_n
        self.repl = np.zeros(4, dtype=np.int32)

    def export(self, hashes, n_blocks, assign, bit_of, key_of, now, ttl, refresh):
        key_by_bit = {int(b): int(k) for b, k in zip(bit_of, key_of)}
        assert len(key_by_bit) == len(bit_of), "cases use distinct bits"
        ent = self.t.entries(hashes, n_blocks, assign, bit_of)
        if self.repl_mutant == "refresh_off_by_one":
            refresh += 1
        if self.repl_mutant == "ignore_liveness":
            ttl = pr.NEVER
        rows = [(h, key_by_bit[bit]) for h, bit in self.t.export(ent, now, ttl, refresh)]
        if self.repl_mutant == "reverse_export":
            rows.reverse()
        self.log_n, kept, dropped = log_append(self.log, self.log_n, rows, self.repl_mutant)
        self.repl[EXPORTED] += kept
        self.repl[DROPPED] += dropped
        return len(ent), len(rows)

    def apply_remote(self, rec, member_keys, member_bits, now, ttl):
        bit_of_key = {int(k): int(b) for k, b in zip(member_keys, member_bits)}
        rec = [(int(h), int(k)) for h, k in np.asarray(rec).reshape(-1, 2)]
        if self.repl_mutant == "apply_unknown_key" and len(member_keys):
            rec = [(h, k if k in bit_of_key else int(member_keys[0])) for h, k in rec]
        applied, skipped = pr.apply_remote(self.t, rec, bit_of_key, now, ttl)
        self.repl[APPLIED] += applied
        self.repl[SKIPPED] += skipped

    def repl_state(self):
        return self.log.copy(), np.array([self.log_n], dtype=np.int32), self.repl.copy()


def run_repl_script(backend, steps) -> list[dict]:
    """State after every step of a script of insert / clear / export /
    apply steps."""
    out = []
    for s in steps:
        snap = {"name": "%s: %s" % (s["op"], s["name"])}
        if s["op"] == "insert":
            backend.insert(s["hashes"], s["n_blocks"], s["assign"], s["bit_of"],
                           s["now"], s["ttl"])
        elif s["op"] == "clear":
            backend.clear_bits(s["mask"])
        elif s["op"] == "export":
            backend.export(s["hashes"], s["n_blocks"], s["assign"], s["bit_of"],
                           s["key_of"], s["now"], s["ttl"], s["refresh"])
        elif s["op"] == "apply":
            backend.apply_remote(s["rec"], s["member_keys"], s["member_bits"],
                                 s["now"], s["ttl"])
        else:
            raise ValueError(s["op"])
        keys, masks, stamps, counters = (pc._np(x) for x in backend.state())
        log, log_n, repl = (pc._np(x) for x in backend.repl_state())
        snap.update(keys=keys.copy(), masks=masks.copy(), stamps=stamps.copy(),
                    counters=counters.copy(), log=log, log_n=log_n, repl=repl)
        out.append(snap)
    return out


FIELDS = ("keys", "masks", "stamps", "counters", "log", "log_n", "repl")


def check_repl_run(got: list[dict], want: list[dict]) -> None:
    """Exact comparison of two run_repl_script results, step by step."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for field in FIELDS:
            a, b = g[field], w[field]
            assert a.shape == b.shape and a.dtype == b.dtype, (w["name"], field)
            bad = np.argwhere(a != b)
            assert bad.size == 0, "step %r: %s differs at %s: got %s want %s" % (
                w["name"], field, bad[:6].tolist(),
                a[tuple(bad[:6].T)].tolist(), b[tuple(bad[:6].T)].tolist())


def rejects(case: dict, mutant: str) -> bool:
    """Whether the comparator tells ``mutant`` from the reference on
    ``case``."""
    want = run_repl_script(RefReplBackend(case["n_buckets"], case["cap"], case["log_n"]),
                           case["steps"])
    got = run_repl_script(
        RefReplBackend(case["n_buckets"], case["cap"], case["log_n"], mutant), case["steps"])
    try:
        check_repl_run(got, want)
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------
# export: the table scripts of prefix_checks, with an export in front of
# every insert
# ---------------------------------------------------------------------------


def export_walk(table: dict) -> dict:
    """pc.table_script(table) as a replication script: before each insert
    step, an export of the same batch (what PrefixIndex.assign does).

    The inserts of that script alone export every entry they bring: each
    batch holds new keys, keys that have expired, or (the last one) a bit
    that clear_bits just removed. So the walk also exports, without
    inserting, at every match step, with replicas cycling over the four
    bits: there the table holds the keys, live or not, with and without the
    bit, young and past the refresh age, and only some entries are
    exported."""
    steps = []
    key_of = keys_of(MEMBERS)
    bit_of = bits_of(pc.REPLICA_BITS)
    for s in pc.table_script(table["batches"], table["max_blocks"]):
        if s["op"] == "clear":
            steps.append(s)
            continue
        ex = dict(op="export", name=s["name"], hashes=s["hashes"], n_blocks=s["n_blocks"],
                  bit_of=bit_of, key_of=key_of, now=s["now"], ttl=s["ttl"],
                  refresh=pr.refresh_of(s["ttl"]))
        if s["op"] == "insert":
            ex["assign"] = s["assign"]
            steps += [ex, s]
        else:
            ex["assign"] = np.arange(len(s["n_blocks"]), dtype=np.int32) % 4
            steps.append(ex)
    return dict(n_buckets=table["n_buckets"], cap=WALK_CAP, log_n=0, steps=steps)


def export_totals(case: dict):
    """(entries, exported before the log's cap) of the reference over the
    case's export steps."""
    ref = RefReplBackend(case["n_buckets"], case["cap"], case["log_n"])
    n_ent = n_exp = 0
    for s in case["steps"]:
        if s["op"] == "export":
            e, x = ref.export(s["hashes"], s["n_blocks"], s["assign"], s["bit_of"],
                              s["key_of"], s["now"], s["ttl"], s["refresh"])
            n_ent, n_exp = n_ent + e, n_exp + x
        else:
            run_repl_script(ref, [s])
    return n_ent, n_exp


# ---------------------------------------------------------------------------
# export: shapes where the compaction can go wrong, and the edges of the
# export rule
# ---------------------------------------------------------------------------


def _export_case(seed, n_blocks, max_blocks, assign=None, *, cap=4096, log_n=0,
                 n_buckets=256, prefill=True, t_insert=5, t_export=(6,), ttl=pc.TTL,
                 refresh=REFRESH) -> dict:
    """A table that knows about half of a batch's blocks (random ones, so
    flags are mixed inside every request), then the batch's export."""
    rng = np.random.default_rng(seed)
    n_req = len(n_blocks)
    h, _ = pc._keys(rng, n_req, max_blocks, max_blocks)
    nb = np.asarray(n_blocks, dtype=np.int32)
    for r in range(n_req):
        h[r, nb[r]:] = 0
    if assign is None:
        assign = np.arange(n_req) % 4
    assign = np.asarray(assign, dtype=np.int32)
    common = dict(n_blocks=nb, assign=assign, bit_of=bits_of(pc.REPLICA_BITS), ttl=ttl)
    steps = []
    if prefill:
        known = h.copy()
        other, _ = pc._keys(rng, n_req, max_blocks, max_blocks)
        swap = rng.random(h.shape) < 0.5
        known[swap] = other[swap]
        steps.append(dict(op="insert", name="half of the batch", hashes=known,
                          now=t_insert, **common))
    for t in t_export:
        steps.append(dict(op="export", name="at %d" % t, hashes=h, key_of=keys_of(MEMBERS),
                          now=t, refresh=refresh, **common))
    return dict(n_buckets=n_buckets, cap=cap, log_n=log_n, steps=steps)


def export_cases() -> dict:
    c = {}
    c["zero_requests"] = _export_case(1, [], 8)
    c["zero_blocks_between_full"] = _export_case(2, [8, 0, 8], 8)
    for mb in (1, 64, 65, 130):
        c["max_blocks_%d" % mb] = _export_case(10 + mb, [mb] * 3, mb, n_buckets=64)
    c["assign_out_of_range"] = _export_case(3, [16] * 6, 16, assign=[0, -1, 1, 4, 2, 3])
    # the flag kernel and the writer take four requests per workgroup
    c["five_requests"] = _export_case(4, [16, 3, 16, 7, 16], 16)
    c["twelve_requests"] = _export_case(5, [70, 1, 0, 64, 65, 70, 2, 70, 63, 0, 5, 70], 70)
    # past 4096 requests a writer workgroup takes more than one group of four
    c["many_requests"] = _export_case(6, [1] * 4100 + [2, 0, 2], 2, cap=8192, n_buckets=1024)
    c["log_n_nonzero"] = _export_case(7, [16] * 4, 16, log_n=37)
    # nothing known: all 48 entries are flagged, 24 fit: the cut is at block
    # 8 of request 1
    c["overflow_mid_request"] = _export_case(8, [16] * 3, 16, cap=24, prefill=False)
    c["overflow_after_log_n"] = _export_case(9, [16] * 3, 16, cap=40, log_n=30)
    c["log_full"] = _export_case(10, [16] * 3, 16, cap=16, log_n=16)
    # the rule's edges: age refresh - 1 against refresh; a dead slot that is
    # younger than refresh (only liveness exports it); ttl 0; ttl NEVER
    c["age_edge"] = _export_case(11, [16] * 4, 16, t_export=(5 + REFRESH - 1, 5 + REFRESH))
    c["dead_under_long_refresh"] = _export_case(12, [16] * 4, 16, ttl=10, refresh=1000,
                                                t_export=(14, 15, 16))
    c["ttl_zero"] = _export_case(13, [16] * 4, 16, ttl=0, refresh=pr.refresh_of(0),
                                 t_export=(5,))
    c["ttl_never"] = _export_case(14, [16] * 4, 16, ttl=pr.NEVER, refresh=pr.NEVER,
                                  t_export=(5, 2 ** 30))
    return c


# ---------------------------------------------------------------------------
# apply_remote
# ---------------------------------------------------------------------------

# the receiver knows r3..r1 under other bits than the sender, and not r0
RECEIVER = dict(member_keys=keys_of(("r3", "r2", "r1", "extra")),
                member_bits=bits_of((0, 63, 5, 32)))


def _records(rng, n, bucket=None, n_buckets=4):
    """n (hash, member key) records over the four sender members (r0 is
    unknown to RECEIVER), every eighth with hash 0, every fifth a repeat of
    an earlier record. ``bucket`` forces every hash into one bucket."""
    h = rng.integers(1, 2 ** 62, n, dtype=np.int64)
    h[rng.random(n) < 0.5] *= -1
    if bucket is not None:
        h = (h & ~np.int64(n_buckets - 1)) | np.int64(bucket)
    k = keys_of(MEMBERS)[rng.integers(0, 4, n)]
    rec = np.stack([h, k], axis=1)
    for i in range(n):
        if i % 8 == 7:
            rec[i, 0] = 0
        elif i % 5 == 4:
            rec[i] = rec[rng.integers(0, i)]
    return rec


def _apply_case(seed, sizes, n_buckets=64, bucket=None, ttl=pc.TTL) -> dict:
    rng = np.random.default_rng(seed)
    steps = [dict(op="apply", name="%d records at %d" % (n, 3 + 2 * i),
                  rec=_records(rng, n, bucket, n_buckets), now=3 + 2 * i, ttl=ttl,
                  **RECEIVER) for i, n in enumerate(sizes)]
    return dict(n_buckets=n_buckets, cap=1, log_n=0, steps=steps)


def apply_cases() -> dict:
    c = {"n_rec_%d" % n: _apply_case(20 + n, [n]) for n in (0, 1, 65, 257)}
    # 3 x 40 records in bucket 1 of a 4-bucket table: 16 slots, so keys are
    # evicted live, oldest first, in list order
    c["one_bucket"] = _apply_case(30, [40, 40, 40], n_buckets=4, bucket=1)
    # entries expire between the rounds: expired slots are reused first
    c["expiring"] = _apply_case(31, [40, 40, 40], n_buckets=4, bucket=2, ttl=2)
    c["no_members"] = _apply_case(32, [65])
    for s in c["no_members"]["steps"]:
        s["member_keys"] = s["member_bits"] = np.zeros(0, dtype=np.int64)
    c["large"] = _apply_case(33, [2000, 2000], n_buckets=1024)
    return c
