"""Reference semantics of the prefix-cache-aware endpoint picker.

Pure Python/numpy, no torch: the normative definition the HIP kernels in
csrc/prefix_kernels.cuh must match bit for bit. There is no floating
point until the final score.

Block hashes. For a request, let t_0..t_{T-1} be its token ids (the entries
of ``out_ids`` that are >= 0, in byte order, inside the request's byte
range). With B = block_tokens and all arithmetic mod 2^64:

    P_j = MUL^(j+1)                       MUL = 0x9E3779B97F4A7C15
    c_k = sum_{j<B} (t_{kB+j} + 1) * P_j  (commutative: any lane order)
    h_-1 = salt;  h_k = mix(h_{k-1} + c_k), 0 remapped to 1

``mix`` is the splitmix64 finaliser. h_k identifies the whole prefix
t_0..t_{(k+1)B-1}. Only full blocks count: n_blocks = min(T // B,
max_blocks).

Table. n_buckets (a power of two) buckets of 16 slots in three arrays:
keys int64, masks int64 (bit i = replica bit i), stamps int32 (whole
seconds). bucket(h) = h & (n_buckets - 1). Key 0 is an empty slot; a slot
is live iff key != 0 and now - stamp < ttl (ttl = NEVER never expires).

Known simplification: a batch is matched before any of its own inserts, so
two new same-prefix requests of one batch do not attract each other.
"""

from __future__ import annotations

import hashlib

import numpy as np

MUL = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
NEVER = 0x7FFFFFFF  # ttl of an index whose slots never expire
SLOTS = 16
MAX_BLOCKS = 256
BLOCK_TOKENS = (8, 16, 32, 64)
N_BITS = 64

# counters[...] of PrefixTable / the device counter block
INSERTED, REFRESHED, REUSED_EXPIRED, EVICTED_LIVE = range(4)


def salt_of(pool) -> int:
    """uint64 salt of a pool name: the first 8 bytes of its SHA-256."""
    if isinstance(pool, str):
        pool = pool.encode("utf-8")
    return int.from_bytes(hashlib.sha256(bytes(pool)).digest()[:8], "little")


def mix(z: int) -> int:
    """splitmix64 finaliser on a uint64."""
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def to_i64(u: int) -> int:
    """uint64 bit pattern as the signed value an int64 array holds."""
    u &= M64
    return u - (1 << 64) if u >> 63 else u


def to_u64(i: int) -> int:
    return int(i) & M64


def powers(block_tokens: int) -> np.ndarray:
    """P_j = MUL^(j+1) for j < block_tokens, as uint64."""
    out, p = [], 1
    for _ in range(block_tokens):
        p = (p * MUL) & M64
        out.append(p)
    return np.array(out, dtype=np.uint64)


def chain(block_sums, salt: int) -> list[int]:
    """h_k (uint64) from the block sums c_k."""
    out, h = [], salt & M64
    for c in block_sums:
        h = mix(h + int(c)) or 1
        out.append(h)
    return out


def token_hashes(tokens, block_tokens: int = 16, max_blocks: int = MAX_BLOCKS,
                 salt: int = 0) -> list[int]:
    """Block hashes (uint64) of one request's token ids."""
    if block_tokens not in BLOCK_TOKENS:
        raise ValueError("block_tokens must be one of %s" % (BLOCK_TOKENS,))
    if not 1 <= max_blocks <= MAX_BLOCKS:
        raise ValueError("max_blocks must be in [1, %d]" % MAX_BLOCKS)
    t = np.asarray(tokens, dtype=np.int64)
    nb = min(len(t) // block_tokens, max_blocks)
    if nb == 0:
        return []
    v = (t[: nb * block_tokens] + 1).astype(np.uint64).reshape(nb, block_tokens)
    with np.errstate(over="ignore"):
        sums = (v * powers(block_tokens)[None, :]).sum(axis=1, dtype=np.uint64)
    return chain(sums.tolist(), salt)


def block_hashes(out_ids, req_off, n_bytes: int, block_tokens: int = 16,
                 max_blocks: int = MAX_BLOCKS, salt: int = 0):
    """(hashes int64[n_req, max_blocks], n_blocks int32[n_req]) of a packed
    batch: request r owns out_ids[req_off[r]:end_r], end_r = req_off[r+1]
    or n_bytes for the last request. Entries past n_blocks are 0."""
    ids = np.asarray(out_ids)
    offs = [int(x) for x in np.asarray(req_off).tolist()]
    n_req = len(offs)
    hashes = np.zeros((n_req, max_blocks), dtype=np.int64)
    n_blocks = np.zeros(n_req, dtype=np.int32)
    for r in range(n_req):
        end = offs[r + 1] if r + 1 < n_req else int(n_bytes)
        seg = ids[offs[r]:min(end, int(n_bytes))]
        hs = token_hashes(seg[seg >= 0], block_tokens, max_blocks, salt)
        n_blocks[r] = len(hs)
        for k, h in enumerate(hs):
            hashes[r, k] = to_i64(h)
    return hashes, n_blocks


class PrefixTable:
    """The block index: which replica bits have seen which block hash."""

    def __init__(self, n_buckets: int):
        if n_buckets < 1 or n_buckets & (n_buckets - 1):
            raise ValueError("n_buckets must be a power of two")
        self.n_buckets = n_buckets
        self.keys = np.zeros(n_buckets * SLOTS, dtype=np.int64)
        self.masks = np.zeros(n_buckets * SLOTS, dtype=np.int64)
        self.stamps = np.zeros(n_buckets * SLOTS, dtype=np.int32)
        self.counters = np.zeros(4, dtype=np.int32)

    def bucket(self, h: int) -> int:
        return to_u64(h) & (self.n_buckets - 1)

    def live(self, slot: int, now: int, ttl: int) -> bool:
        return self.keys[slot] != 0 and int(now) - int(self.stamps[slot]) < int(ttl)

    def block_mask(self, h: int, live_mask: int, now: int, ttl: int) -> int:
        """mask_k: OR of the masks of the live slots holding h, ANDed with
        live_mask (uint64)."""
        h = to_i64(h)
        base = self.bucket(h) * SLOTS
        m = 0
        for s in range(base, base + SLOTS):
            if self.keys[s] == h and self.live(s, now, ttl):
                m |= to_u64(self.masks[s])
        return m & to_u64(live_mask)

    def match(self, hashes, n_blocks, live_mask: int, now: int, ttl: int) -> np.ndarray:
        """matched int32[n_req, 64]: per replica bit, the length of the
        leading run of the request's blocks that the bit has seen. A block
        missing in the middle ends the run."""
        hashes = np.asarray(hashes, dtype=np.int64)
        out = np.zeros((hashes.shape[0], N_BITS), dtype=np.int32)
        for r in range(hashes.shape[0]):
            acc = M64
            for k in range(int(n_blocks[r])):
                acc &= self.block_mask(int(hashes[r, k]), live_mask, now, ttl)
                if not acc:
                    break
                for i in range(N_BITS):
                    out[r, i] += (acc >> i) & 1
        return out

    def entries(self, hashes, n_blocks, assign, bit_of) -> list[tuple[int, int]]:
        """The insert list, request-major and block-minor: (h, bit) as
        signed int64 values."""
        hashes = np.asarray(hashes, dtype=np.int64)
        out = []
        for r in range(hashes.shape[0]):
            a = int(assign[r])
            if a < 0 or a >= len(bit_of):
                continue
            for k in range(int(n_blocks[r])):
                if hashes[r, k] != 0:
                    out.append((int(hashes[r, k]), to_i64(int(bit_of[a]))))
        return out

    def insert(self, hashes, n_blocks, assign, bit_of, now: int, ttl: int) -> None:
        self.apply(self.entries(hashes, n_blocks, assign, bit_of), now, ttl)

    def apply(self, entries, now: int, ttl: int) -> None:
        """Apply (h, bit) entries in list order. Buckets do not interact,
        so only the order inside one bucket matters."""
        cnt = self.counters
        for h, bit in entries:
            base = self.bucket(h) * SLOTS
            slots = range(base, base + SLOTS)
            hit = next((s for s in slots if self.keys[s] == h), None)
            if hit is not None:
                if self.live(hit, now, ttl):
                    self.masks[hit] |= np.int64(bit)
                else:
                    self.masks[hit] = bit
                    cnt[REUSED_EXPIRED] += 1
                self.stamps[hit] = now
                cnt[REFRESHED] += 1
                continue
            victim = next((s for s in slots if self.keys[s] == 0), None)
            if victim is None:
                victim = next((s for s in slots if not self.live(s, now, ttl)), None)
                if victim is not None:
                    cnt[REUSED_EXPIRED] += 1
                else:
                    victim = min(slots, key=lambda s: (int(self.stamps[s]), s))
                    cnt[EVICTED_LIVE] += 1
            self.keys[victim] = h
            self.masks[victim] = bit
            self.stamps[victim] = now
            cnt[INSERTED] += 1

    def clear_bits(self, mask: int) -> None:
        self.masks &= np.int64(to_i64(~to_u64(mask)))

    def export(self, entries, now: int, ttl: int, refresh: int) -> list[tuple[int, int]]:
        """The entries of an insert list that other shards need to hear of,
        judged against the table as it stands BEFORE the list is applied.
        With s the slot of bucket(h) whose key is h, (h, bit) is exported
        iff there is no such slot, or s is not live, or masks[s] lacks bit,
        or now - stamps[s] >= refresh (the origin re-announces an entry it
        keeps refreshing, or it would expire elsewhere while still hot).
        Input order is kept, duplicates included: applying is idempotent."""
        out = []
        for h, bit in entries:
            base = self.bucket(h) * SLOTS
            s = next((s for s in range(base, base + SLOTS) if self.keys[s] == h), None)
            if (s is None or not self.live(s, now, ttl)
                    or to_u64(self.masks[s]) & to_u64(bit) == 0
                    or int(now) - int(self.stamps[s]) >= int(refresh)):
                out.append((h, bit))
        return out


def member_key(name) -> int:
    """uint64 identity of a pool member on every shard: the first 8 bytes
    of the SHA-256 of its name, 0 remapped to 1. Shards hand out replica
    bits in their own order; the key is what travels."""
    if isinstance(name, str):
        name = name.encode("utf-8")
    return int.from_bytes(hashlib.sha256(bytes(name)).digest()[:8], "little") or 1


def refresh_of(ttl: int) -> int:
    """Age at which the origin exports a live entry again: half its TTL."""
    return NEVER if ttl == NEVER else max(int(ttl) // 2, 1)


def apply_remote(table: PrefixTable, records, bit_of_key: dict, now: int,
                 ttl: int) -> tuple[int, int]:
    """Apply another shard's exported (h, member_key) records: (applied,
    skipped). A record with h == 0 or a key this shard does not know is
    skipped; the rest go through PrefixTable.apply in list order under the
    receiver's own ``now`` (stamps never travel: every index has its own
    clock). Keys are compared as uint64 bit patterns."""
    known = {to_u64(k): b for k, b in bit_of_key.items()}
    entries, skipped = [], 0
    for h, key in records:
        bit = known.get(to_u64(key))
        if int(h) == 0 or bit is None:
            skipped += 1
            continue
        entries.append((to_i64(int(h)), to_i64(int(bit))))
    table.apply(entries, now, ttl)
    return len(entries), skipped


def score_assign(stats, pred, matched, block_tokens: int, weights, dtype=np.float32):
    """Greedy assignment with the prefix-hit term, evaluated in ``dtype``.
    matched[i][lane] is in stats-row (lane) order. Per request and lane:
    hit = min(matched * B, p); p_eff = p - hit; score = w_kv * (1 - (used +
    p_eff) / max(cap, 1)) - w_q * queue - w_a * active + w_p * hit /
    max(p, 1), minus 1e6 when used + p_eff > cap. The lowest lane wins
    ties; the winner absorbs p_eff, +1 queue and +1 active."""
    f = dtype
    s = np.array(stats, dtype=f).copy()
    w_kv, w_q, w_a, w_p = (f(w) for w in weights)
    matched = np.asarray(matched)
    out = []
    for i, p in enumerate(np.asarray(pred, dtype=f)):
        best, best_score, best_eff = -1, None, f(0)
        for r in range(s.shape[0]):
            used, cap, queue, active = s[r]
            hit = min(f(int(matched[i][r]) * block_tokens), p)
            p_eff = p - hit
            sc = (w_kv * (f(1) - (used + p_eff) / max(cap, f(1))) - w_q * queue
                  - w_a * active + w_p * hit / max(p, f(1)))
            if used + p_eff > cap:
                sc = sc - f(1e6)
            if best_score is None or sc > best_score:
                best, best_score, best_eff = r, sc, p_eff
        out.append(best)
        s[best, 0] += best_eff
        s[best, 2] += f(1)
        s[best, 3] += f(1)
    return out
