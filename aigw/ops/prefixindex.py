"""HBM-resident prefix block index of one replica pool.

Holds, per chained token-block hash, the 64-bit mask of the replicas that
have been sent a prompt starting with that block chain. The admission
path's on-device BPE token ids are hashed, matched against the table and
folded into the greedy endpoint scorer without leaving the GPU; the pick
is then recorded in the table. Semantics: aigw/ops/prefix_ref.py.

A batch is matched before any of its own inserts, so two new same-prefix
requests of one batch do not attract each other.

With ``replicate=True`` the index also logs, on the device, the inserts
the node's other shards need to hear of, as (hash, member key) records: a
member's key is the same on every shard, its bit is not. StateSync drains
the log on its tick and applies the other shards' records here.
"""

from __future__ import annotations

import time
from typing import Optional, Sequence

import torch

from aigw.ops import load_hip_module
from aigw.ops.prefix_ref import (
    BLOCK_TOKENS, MAX_BLOCKS, N_BITS, NEVER, SLOTS, member_key, refresh_of, salt_of,
    to_i64,
)

SCORE_WEIGHTS = (1.0, 0.1, 0.05)  # w_kv, w_q, w_a of pick_endpoint
LOG_RECORDS = 65536  # replication log rows of (hash, member key): 1 MiB


class PrefixIndex:
    def __init__(
        self,
        pool: str,
        *,
        block_tokens: int = 16,
        max_blocks: int = 256,
        buckets: int = 65536,
        ttl_s: Optional[float] = 300.0,  # None: entries never expire
        weight: float = 1.0,
        replicate: bool = False,  # log inserts for the other shards
        device: str = "cuda",
        _hip=None,
        _clock=time.monotonic,
    ):
        if block_tokens not in BLOCK_TOKENS:
            raise ValueError("block_tokens must be one of %s" % (BLOCK_TOKENS,))
        if not 1 <= max_blocks <= MAX_BLOCKS:
            raise ValueError("max_blocks must be in [1, %d]" % MAX_BLOCKS)
        if buckets < 1 or buckets & (buckets - 1):
            raise ValueError("buckets must be a power of two")
        self.hip = _hip if _hip is not None else load_hip_module()
        if self.hip is None:
            raise RuntimeError("aigw_hip extension unavailable")
        self.pool = pool
        self.device = torch.device(device)
        self.block_tokens = block_tokens
        self.max_blocks = max_blocks
        self.n_buckets = buckets
        self.weight = float(weight)
        self.salt = to_i64(salt_of(pool))
        if ttl_s is None or ttl_s == float("inf"):
            self.ttl = NEVER
        else:
            self.ttl = int(min(max(ttl_s, 0), NEVER))
        n = buckets * SLOTS
        self.keys = torch.zeros(n, dtype=torch.int64, device=self.device)
        self.masks = torch.zeros(n, dtype=torch.int64, device=self.device)
        self.stamps = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.counters = torch.zeros(4, dtype=torch.int32, device=self.device)
        # whole seconds of the index's own clock, which starts at 0 when
        # the index is built (as SemanticCache.now())
        self._clock = _clock
        self._t0 = _clock()
        # stable member name -> bit; a vanished member's bit is retired and
        # cleared from the table before another member may take it
        self._bit: dict[str, int] = {}
        self._retired: list[int] = []
        self._free: list[int] = list(range(N_BITS))
        # device copies of the last member list's bits (pools change rarely)
        self._dev_key: Optional[tuple] = None
        self._dev_cols = self._dev_bit_of = None
        # replication: the batch's entries that other shards need are
        # appended on the device as (hash, member key) rows; drain_log()
        # hands them to the state-sync tick, apply_remote() takes theirs
        self.replicate = bool(replicate)
        self.refresh = refresh_of(self.ttl)
        self.repl_counters = torch.zeros(4, dtype=torch.int32, device=self.device)
        self.log = self.log_n = None
        if self.replicate:
            self.log = torch.zeros(LOG_RECORDS, 2, dtype=torch.int64, device=self.device)
            self.log_n = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._dev_names: Optional[tuple] = None
        self._dev_key_of = None
        self._dev_members: Optional[tuple] = None
        self._dev_member_keys = self._dev_member_bits = None

    def now(self) -> int:
        return int(min(max(self._clock() - self._t0, 0.0), NEVER - 1))

    # ---- member bits -----------------------------------------------------

    @property
    def live_mask(self) -> int:
        m = 0
        for b in self._bit.values():
            m |= 1 << b
        return to_i64(m)

    def set_members(self, members: Sequence[str]) -> list[int]:
        """Make ``members`` the live set and return each one's bit."""
        want = list(members)
        if len(set(want)) != len(want):
            raise ValueError("duplicate member names")
        if len(want) > N_BITS:
            raise ValueError("a prefix index holds at most %d live members" % N_BITS)
        if len(want) != len(self._bit) or any(m not in self._bit for m in want):
            keep = set(want)
            for name in [n for n in self._bit if n not in keep]:
                self._retired.append(self._bit.pop(name))
            for name in want:
                if name not in self._bit:
                    self._bit[name] = self._take_bit()
        return [self._bit[m] for m in want]

    def _take_bit(self) -> int:
        if not self._free:
            # hand retired bits out again only after clearing them from
            # every mask, so the new member inherits nobody's blocks
            mask = 0
            for b in self._retired:
                mask |= 1 << b
            self.clear_bits(to_i64(mask))
            self._free, self._retired = sorted(self._retired), []
        if not self._free:
            raise ValueError("a prefix index holds at most %d live members" % N_BITS)
        return self._free.pop(0)

    # ---- device ops ------------------------------------------------------

    def hashes(self, out_ids: torch.Tensor, req_off: torch.Tensor, n_bytes: int):
        """(hashes int64[n_req, max_blocks], n_blocks int32[n_req])."""
        return self.hip.prefix_block_hashes(
            out_ids, req_off, int(n_bytes), self.block_tokens, self.max_blocks, self.salt
        )

    def match(self, hashes: torch.Tensor, n_blocks: torch.Tensor,
              now: Optional[int] = None) -> torch.Tensor:
        """int32[n_req, 64]: per member bit, the leading run of blocks."""
        return self.hip.prefix_match(
            self.keys, self.masks, self.stamps, hashes, n_blocks, self.live_mask,
            self.now() if now is None else now, self.ttl,
        )

    def _dev_bits(self, bits: Sequence[int]):
        key = tuple(bits)
        if key != self._dev_key:
            self._dev_cols = torch.tensor(list(key), dtype=torch.int64, device=self.device)
            self._dev_bit_of = torch.tensor([to_i64(1 << b) for b in key],
                                            dtype=torch.int64, device=self.device)
            self._dev_key = key
        return self._dev_cols, self._dev_bit_of

    def insert(self, hashes: torch.Tensor, n_blocks: torch.Tensor,
               assign: torch.Tensor, bits: Sequence[int],
               now: Optional[int] = None) -> None:
        """Record request r's blocks under bit ``bits[assign[r]]``."""
        bit_of = self._dev_bits(bits)[1]
        self.hip.prefix_insert(
            self.keys, self.masks, self.stamps, self.counters, hashes, n_blocks,
            assign, bit_of, self.now() if now is None else now, self.ttl,
        )

    def clear_bits(self, mask: int) -> None:
        self.hip.prefix_clear_bits(self.masks, mask)

    # ---- replication -----------------------------------------------------

    def _dev_keys(self, members: Sequence[str]) -> torch.Tensor:
        """member_key of each member, in ``members`` (stats row) order."""
        names = tuple(members)
        if names != self._dev_names:
            self._dev_key_of = torch.tensor([to_i64(member_key(m)) for m in names],
                                            dtype=torch.int64, device=self.device)
            self._dev_names = names
        return self._dev_key_of

    def export(self, hashes: torch.Tensor, n_blocks: torch.Tensor, assign: torch.Tensor,
               members: Sequence[str], bits: Sequence[int],
               now: Optional[int] = None) -> None:
        """Append the batch's entries that other shards need to hear of to
        the log; to be called before insert() of the same batch. No host
        sync."""
        if not self.replicate:
            raise RuntimeError("PrefixIndex was built with replicate=False")
        self.hip.prefix_export(
            self.keys, self.masks, self.stamps, hashes, n_blocks, assign,
            self._dev_bits(bits)[1], self._dev_keys(members), self.log, self.log_n,
            self.repl_counters, self.now() if now is None else now, self.ttl, self.refresh,
        )

    def drain_log(self, max_n: int) -> torch.Tensor:
        """The oldest <= max_n log records as int64[k, 2] rows of (hash,
        member key) on the device; the rest stay, in FIFO order. The only
        place that reads log_n on the host: one sync per tick, off the
        request path."""
        if not self.replicate:
            return torch.zeros(0, 2, dtype=torch.int64, device=self.device)
        n = int(self.log_n.item())
        k = max(min(n, int(max_n)), 0)
        out = self.log[:k].clone()
        if k:
            if k < n:
                self.log[: n - k] = self.log[k:n].clone()
            self.log_n.fill_(n - k)
        return out

    def apply_remote(self, rec: torch.Tensor, now: Optional[int] = None) -> None:
        """Apply another shard's drained records under this index's own
        bits and clock. Records of members unknown here are skipped."""
        rec = rec.to(self.device, torch.int64).contiguous()
        live = tuple(sorted(self._bit.items(), key=lambda nb: nb[1]))
        if live != self._dev_members:
            self._dev_member_keys = torch.tensor(
                [to_i64(member_key(name)) for name, _ in live],
                dtype=torch.int64, device=self.device)
            self._dev_member_bits = torch.tensor(
                [to_i64(1 << b) for _, b in live], dtype=torch.int64, device=self.device)
            self._dev_members = live
        self.hip.prefix_apply_remote(
            self.keys, self.masks, self.stamps, self.counters, rec, rec.shape[0],
            self._dev_member_keys, self._dev_member_bits, self.repl_counters,
            self.now() if now is None else now, self.ttl,
        )

    def assign(self, members: Sequence[str], stats: torch.Tensor,
               predicted: torch.Tensor, out_ids: torch.Tensor,
               req_off: torch.Tensor, n_bytes: int):
        """hash -> match -> score -> (export, when replicating) -> insert
        for one batch, all on the current stream with no host sync.
        Returns device tensors
        (assign int32[n_req], hit_blocks int32[n_req], n_blocks): hit_blocks
        is the matched run on the replica each request went to."""
        bits = self.set_members(members)
        now = self.now()
        hashes, n_blocks = self.hashes(out_ids, req_off, n_bytes)
        matched = self.match(hashes, n_blocks, now)
        cols = self._dev_bits(bits)[0]
        by_lane = matched.index_select(1, cols).contiguous()  # bit -> stats row order
        w_kv, w_q, w_a = SCORE_WEIGHTS
        assign = self.hip.kv_score_assign_prefix(
            stats, predicted, by_lane, self.block_tokens, w_kv, w_q, w_a, self.weight
        )
        if self.replicate:  # judged against the table before this batch's inserts
            self.export(hashes, n_blocks, assign, members, bits, now)
        self.insert(hashes, n_blocks, assign, bits, now)
        hit = by_lane.gather(1, assign.to(torch.int64).unsqueeze(1)).squeeze(1)
        return assign, hit, n_blocks

    def stats(self) -> dict:
        c = self.counters.cpu().tolist()
        r = self.repl_counters.cpu().tolist()
        return {
            "inserted": c[0], "refreshed": c[1], "reused_expired": c[2],
            "evicted_live": c[3], "members": len(self._bit),
            "exported": r[0], "dropped": r[1], "applied": r[2], "skipped": r[3],
        }
