"""Cases, backends and comparators for the prefix-picker kernels.

One scripted scenario runs against any backend: the reference
(aigw.ops.prefix_ref), a deliberately wrong emulation of it (a "mutant"),
or the HIP kernels. The comparators demand exact equality with the
reference after every step; tests/test_prefix_ref_cpu.py shows on the CPU
that they reject every mutant on these very cases, so a GPU pass means
something.
"""

from __future__ import annotations

import numpy as np

from aigw.ops import prefix_ref as pr

VOCAB = 33024  # 256 bytes + 32768 merges: the default tokenizer's ids

# ---------------------------------------------------------------------------
# block hashes
# ---------------------------------------------------------------------------

HASH_PATTERNS = ("dense", "alternate", "long_hole")
HASH_MUTANTS = ("drop_last_chunk", "partial_block", "no_chain")


def token_counts(block_tokens: int, max_blocks: int) -> list[int]:
    b, full = block_tokens, max_blocks * block_tokens
    return [0, 1, b - 1, b, b + 1, 2 * b - 1, 255, 256, 257, full, full + 1]


def _place(tokens: np.ndarray, pattern: str, rng) -> np.ndarray:
    """One request's slice of out_ids: its tokens in order, -1 elsewhere."""
    n = len(tokens)
    if pattern == "dense":
        return tokens.astype(np.int32)
    if pattern == "alternate":  # a hole after every token
        out = np.full(2 * n, -1, dtype=np.int32)
        out[0::2] = tokens
        return out
    if pattern == "long_hole":
        # a hole run longer than two chunks after the first few tokens, so
        # some 256-position chunk holds no token wherever the request
        # starts; a short hole run at the end
        head = min(n, 5)
        return np.concatenate([
            tokens[:head].astype(np.int32), np.full(600, -1, dtype=np.int32),
            tokens[head:].astype(np.int32), np.full(3, -1, dtype=np.int32),
        ])
    raise ValueError(pattern)


def hash_batch(block_tokens: int, max_blocks: int, pattern: str, seed: int = 0):
    """(out_ids int32, req_off int64, n_bytes): one request per token count
    of token_counts(), packed back to back so request boundaries fall
    inside chunks, plus an empty request (no bytes at all) in the middle.
    The last request ends at n_bytes."""
    rng = np.random.default_rng(1000 * block_tokens + max_blocks + seed)
    parts, offs, off = [], [], 0
    counts = token_counts(block_tokens, max_blocks)
    order = rng.permutation(len(counts)).tolist()
    for j, ci in enumerate(order):
        if j == len(order) // 2:
            offs.append(off)  # the empty request: lo == hi
        seg = _place(rng.integers(0, VOCAB, counts[ci]), pattern, rng)
        offs.append(off)
        parts.append(seg)
        off += len(seg)
    out_ids = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
    return out_ids, np.array(offs, dtype=np.int64), int(off)


def big_request_batch(block_tokens: int = 64, max_blocks: int = 256):
    """A 256 KiB request with a token every 16 bytes: 16384 tokens, which is
    256 full blocks of 64, so the whole range is walked. A short request
    follows it."""
    rng = np.random.default_rng(77)
    n = 262144
    out = np.full(n + 40, -1, dtype=np.int32)
    out[0:n:16] = rng.integers(0, VOCAB, n // 16)
    out[n:] = rng.integers(0, VOCAB, 40)
    return out, np.array([0, n], dtype=np.int64), n + 40


def emulate_hashes(out_ids, req_off, n_bytes, block_tokens, max_blocks, salt,
                   mutant=None):
    """The kernel's algorithm on the CPU: walk each request in 256-position
    chunks with a running token count, add into per-block sums, chain at
    the end. ``mutant`` plants one of HASH_MUTANTS."""
    ids = np.asarray(out_ids)
    offs = [int(x) for x in req_off]
    pw = [int(x) for x in pr.powers(block_tokens)]
    cap = max_blocks * block_tokens
    n_req = len(offs)
    hashes = np.zeros((n_req, max_blocks), dtype=np.int64)
    n_blocks = np.zeros(n_req, dtype=np.int32)
    for r in range(n_req):
        lo = offs[r]
        hi = min(offs[r + 1] if r + 1 < n_req else n_bytes, n_bytes)
        c = [0] * (max_blocks + 1)
        running = 0
        base = lo
        while base < hi and running < cap:
            end = min(base + 256, hi)
            if mutant == "drop_last_chunk" and end == hi and end - base < 256:
                break
            for pos in range(base, end):
                t = int(ids[pos])
                if t >= 0:
                    if running < cap:
                        c[running // block_tokens] += (t + 1) * pw[running % block_tokens]
                    running += 1
            base += 256
        nb = running // block_tokens
        if mutant == "partial_block" and running % block_tokens:
            nb += 1
        nb = min(nb, max_blocks)
        n_blocks[r] = nb
        h = salt & pr.M64
        for k in range(nb):
            h = pr.mix((salt if mutant == "no_chain" else h) + c[k]) or 1
            hashes[r, k] = pr.to_i64(h)
    return hashes, n_blocks


def _np(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def check_hashes(hashes, n_blocks, out_ids, req_off, n_bytes, block_tokens,
                 max_blocks, salt) -> dict:
    """Exact comparison with prefix_ref.block_hashes; raises on any
    difference. Returns how much the case exercised."""
    want_h, want_n = pr.block_hashes(out_ids, req_off, n_bytes, block_tokens,
                                     max_blocks, salt)
    got_h, got_n = _np(hashes), _np(n_blocks)
    assert got_n.dtype == np.int32 and got_h.dtype == np.int64
    assert got_h.shape == want_h.shape and got_n.shape == want_n.shape
    bad = np.nonzero(got_n != want_n)[0]
    assert bad.size == 0, "n_blocks differs at requests %s: got %s want %s" % (
        bad[:8].tolist(), got_n[bad[:8]].tolist(), want_n[bad[:8]].tolist())
    bad = np.argwhere(got_h != want_h)
    assert bad.size == 0, "hashes differ at (request, block) %s" % bad[:8].tolist()
    return {"requests": int(len(want_n)), "blocks": int(want_n.sum())}


# ---------------------------------------------------------------------------
# table: insert / match / clear_bits
# ---------------------------------------------------------------------------

TABLE_MUTANTS = ("ttl_off_by_one", "lose_bit63", "ignore_live_mask", "reverse_inserts")
REPLICA_BITS = (0, 31, 32, 63)
ALL_BITS = pr.M64
TTL = 100


class RefBackend:
    """prefix_ref.PrefixTable behind the backend interface, optionally with
    one of TABLE_MUTANTS planted."""

    def __init__(self, n_buckets: int, mutant=None):
        self.t = pr.PrefixTable(n_buckets)
        self.mutant = mutant

    def _ttl(self, ttl):
        return ttl + 1 if self.mutant == "ttl_off_by_one" else ttl

    def match(self, hashes, n_blocks, live_mask, now, ttl):
        if self.mutant == "ignore_live_mask":
            live_mask = ALL_BITS
        if self.mutant == "lose_bit63":
            live_mask &= ~(1 << 63)
        return self.t.match(hashes, n_blocks, live_mask, now, self._ttl(ttl))

    def insert(self, hashes, n_blocks, assign, bit_of, now, ttl):
        ent = self.t.entries(hashes, n_blocks, assign, bit_of)
        if self.mutant == "reverse_inserts":
            ent.reverse()
        self.t.apply(ent, now, self._ttl(ttl))

    def clear_bits(self, mask):
        self.t.clear_bits(mask)

    def state(self):
        return (self.t.keys.copy(), self.t.masks.copy(), self.t.stamps.copy(),
                self.t.counters.copy())


def _keys(rng, n_req, n_blk, max_blocks):
    h = rng.integers(1, 2 ** 63 - 1, (n_req, max_blocks), dtype=np.int64)
    h[rng.random((n_req, max_blocks)) < 0.5] *= -1  # both signs: bit 63 of a key
    nb = np.full(n_req, n_blk, dtype=np.int32)
    h[:, n_blk:] = 0
    return h, nb


def table_script(batches, max_blocks: int, seed: int = 5) -> list[dict]:
    """The scenario both tables run. ``batches`` is a list of (n_req,
    n_blocks) giving the number of new keys each insert brings."""
    rng = np.random.default_rng(seed)
    bit_of = np.array([pr.to_i64(1 << b) for b in REPLICA_BITS], dtype=np.int64)
    steps: list[dict] = []

    def ins(name, h, nb, assign, now):
        steps.append(dict(op="insert", name=name, hashes=h, n_blocks=nb,
                          assign=np.asarray(assign, dtype=np.int32), bit_of=bit_of,
                          now=now, ttl=TTL))

    def mat(name, h, nb, now, live_mask=ALL_BITS, ttl=TTL):
        steps.append(dict(op="match", name=name, hashes=h, n_blocks=nb,
                          live_mask=pr.to_i64(live_mask), now=now, ttl=ttl))

    (na, ba), rest = batches[0], batches[1:]
    ha, nba = _keys(rng, na, ba, max_blocks)
    # batch A: replicas cycle over bits 0/31/32/63; request 1 is dropped
    # (assign -1); request 2 has no full block; the last request repeats
    # request 0's blocks under another replica (one key, two replicas, one
    # batch); request 3 shares request 0's first half only
    ha[-1] = ha[0]
    half = max(ba // 2, 1)
    ha[3, :half] = ha[0, :half]
    nba[2] = 0
    assign_a = [i % 4 for i in range(na)]
    assign_a[1] = -1
    assign_a[0], assign_a[-1] = 3, 1  # bits 63 and 31 on the same keys
    mat("empty table", ha, nba, 10)
    ins("batch A", ha, nba, assign_a, 10)
    mat("after A", ha, nba, 10)
    broken = ha.copy()
    broken[:, half] = rng.integers(1, 2 ** 62, na)  # a block nobody has seen
    mat("run broken in the middle", broken, nba, 10)
    mat("ttl edge: last live second", ha, nba, 10 + TTL - 1)
    mat("ttl edge: dead", ha, nba, 10 + TTL)
    mat("never expires", ha, nba, 10 + TTL + 5, ttl=pr.NEVER)
    mat("live_mask without bit 63", ha, nba, 10, live_mask=ALL_BITS & ~(1 << 63))
    mat("live_mask of bit 31 only", ha, nba, 10, live_mask=1 << 31)
    # A's keys again after they expired, under shifted replicas: masks are
    # reset, not ORed
    now = 10 + TTL
    ins("A again, expired", ha, nba, [(a + 1) % 4 if a >= 0 else -1 for a in assign_a], now)
    mat("after expired re-insert", ha, nba, now)
    # new keys at later seconds: empty slots first, then (once A's entries
    # expire again) expired ones, else the oldest stamp
    seen = [(ha, nba)]
    for j, (n_req, n_blk) in enumerate(rest):
        now += 7
        h, nb = _keys(rng, n_req, n_blk, max_blocks)
        ins("batch %d" % (j + 1), h, nb, [i % 4 for i in range(n_req)], now)
        seen.append((h, nb))
        for hs, nbs in seen:
            mat("after batch %d" % (j + 1), hs, nbs, now)
    steps.append(dict(op="clear", name="clear bits 32 and 63",
                      mask=pr.to_i64((1 << 32) | (1 << 63))))
    for hs, nbs in seen:
        mat("after clear_bits", hs, nbs, now)
    # refresh live keys: OR a new bit in, same second and a later one
    ins("refresh", seen[-1][0], seen[-1][1], [2] * len(seen[-1][1]), now + 1)
    mat("after refresh", seen[-1][0], seen[-1][1], now + 1)
    return steps


SMALL_TABLE = dict(n_buckets=4, max_blocks=130,
                   batches=[(6, 8), (3, 8), (1, 130), (2, 8)])  # ~200 keys
LARGE_TABLE = dict(n_buckets=1024, max_blocks=16,
                   batches=[(128, 16), (64, 16), (32, 16), (32, 16)])  # 4096 keys


def run_script(backend, steps) -> list[dict]:
    """State after every step: the table arrays, the counters, and the
    match result of a match step."""
    out = []
    for s in steps:
        snap = {"name": "%s: %s" % (s["op"], s["name"])}
        if s["op"] == "insert":
            backend.insert(s["hashes"], s["n_blocks"], s["assign"], s["bit_of"],
                           s["now"], s["ttl"])
        elif s["op"] == "match":
            snap["matched"] = _np(backend.match(s["hashes"], s["n_blocks"],
                                                s["live_mask"], s["now"], s["ttl"]))
        else:
            backend.clear_bits(s["mask"])
        keys, masks, stamps, counters = (_np(x) for x in backend.state())
        snap.update(keys=keys, masks=masks, stamps=stamps, counters=counters)
        out.append(snap)
    return out


def check_run(got: list[dict], want: list[dict]) -> dict:
    """Exact comparison of two run_script results, step by step."""
    assert len(got) == len(want)
    n_match = 0
    for g, w in zip(got, want):
        for field in ("keys", "masks", "stamps", "counters", "matched"):
            if field not in w:
                continue
            a, b = g[field], w[field]
            assert a.shape == b.shape and a.dtype == b.dtype, (w["name"], field)
            bad = np.argwhere(a != b)
            assert bad.size == 0, "step %r: %s differs at %s: got %s want %s" % (
                w["name"], field, bad[:6].tolist(),
                a[tuple(bad[:6].T)].tolist(), b[tuple(bad[:6].T)].tolist())
        n_match += "matched" in w
    return {"steps": len(want), "matches": n_match}


# ---------------------------------------------------------------------------
# scorer
# ---------------------------------------------------------------------------

PREFIX_WEIGHTS = (1.0, 0.125, 0.0625, 1.0)  # w_kv, w_q, w_a, w_p
SCORE_BLOCK = 16


def prefix_kv_cases() -> dict:
    """name -> (stats rows, pred, matched int32[n_req, n_rep]). Built as
    kernel_checks.kv_cases(): integers, power-of-two predictions and
    capacities, so every intermediate of the score is exact in fp32 (the
    tests assert fp32 == fp64 before trusting either). hit/p is a multiple
    of 1/p >= 2^-12 and the occupancy term a multiple of 2^-16, with
    |score| < 16: 20 bits, inside fp32's 24."""
    rng = np.random.default_rng(21)
    cases = {}
    idle = [0.0, 65536.0, 0.0, 0.0]
    # affinity overrides load: replica 2 is a little busier but holds the
    # whole prompt (+1 for the hit against -0.1875 for one queued request)
    rows = [list(idle) for _ in range(4)]
    rows[2] = [1024.0, 65536.0, 1.0, 1.0]
    m = np.zeros((1, 4), dtype=np.int32)
    m[0, 2] = 64
    cases["affinity_over_load"] = (rows, np.array([1024.0]), m)
    # load overrides affinity: 40 queued requests cost 7.5, the hit gives 1
    rows = [list(idle) for _ in range(4)]
    rows[2] = [1024.0, 65536.0, 40.0, 40.0]
    cases["load_over_affinity"] = (rows, np.array([1024.0]), m.copy())
    # hit > p: 64 matched blocks are 1024 tokens against a predicted 256;
    # the hit is capped at p and the replica is charged nothing
    rows = [list(idle) for _ in range(4)]
    rows[3] = [65536.0 - 128.0, 65536.0, 0.0, 0.0]  # fits only with the hit
    m3 = np.zeros((2, 4), dtype=np.int32)
    m3[:, 3] = 64
    cases["hit_over_p"] = (rows, np.array([256.0, 256.0]), m3)
    for n_rep in (1, 2, 63, 64):
        n_req = 64
        # one or two replicas must never overflow (a penalised score is not
        # exact in fp32): 64 predictions of at most 2^10 against 2^18
        small = n_rep <= 2
        pred = (2.0 ** rng.integers(6, 11 if small else 13, n_req)).astype(np.float64)
        rows = []
        for _ in range(n_rep):
            cap = float(2 ** (18 if small else int(rng.integers(14, 17))))
            rows.append([float(rng.integers(0, int(cap) // 4)), cap,
                         float(rng.integers(0, 7)), float(rng.integers(0, 7))])
        if n_rep > 2:
            rows[0] = [0.0, 0.0, 0.0, 0.0]  # zero capacity: always penalised
            rows[1] = [0.0, 2.0 ** 18, 8.0, 8.0]  # always fits: a clean winner exists
        # runs of up to twice the prompt's blocks, so hit > p occurs; most
        # entries zero, as in a real table
        mm = rng.integers(0, 2 * (pred[:, None] / SCORE_BLOCK).astype(np.int64) + 1,
                          (n_req, n_rep)).astype(np.int32)
        mm[rng.random((n_req, n_rep)) < 0.6] = 0
        cases[f"mixed_{n_rep}"] = (rows, pred, mm)
    return cases
