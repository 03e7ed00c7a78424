"""Semantic response cache: MFMA embedding + HBM-resident cosine index.

The embedding pipeline (mean-pooled token embeddings → bf16 MFMA projection
→ L2 normalize) runs entirely on the GPU from the tokenizer's on-device
output. The index is a ring buffer of bf16 rows sized for the 288 GB HBM3E
budget; lookup is the fused MFMA similarity + argmax kernel (one pass over
the index, no materialized score matrix).
"""

from __future__ import annotations

import hashlib
import math
import time
from typing import Optional

import torch

from aigw.ops import load_hip_module


NEVER = 0x7FFFFFFF  # row_expiry of a row without a TTL


def scope_id(b: bytes) -> int:
    """Index scope id of a scope tag: the first 8 bytes of its SHA-256 as a
    signed int64, with 0 (the lookup wildcard) remapped to 1. Two tags may
    share an id; callers that must never cross scopes keep comparing the
    full tag on the value, so a collision costs a miss, not a leak."""
    v = int.from_bytes(hashlib.sha256(b).digest()[:8], "little", signed=True)
    return v or 1


class SemanticCache:
    scope_id = staticmethod(scope_id)

    def __init__(
        self,
        vocab_size: int,
        dim: int = 384,
        capacity: int = 65536,
        threshold: float = 0.92,
        device: str = "cuda",
        seed: int = 7,
        index_dtype: str = "bf16",  # "bf16" | "fp8" (OCP e4m3: half the
        # HBM per row -> 2x rows in the 288 GB budget, 2x lookup bandwidth;
        # ~1% cosine error from 3-bit mantissas averaged over 384 dims)
        _hip=None,
        *,
        scoped: bool = False,  # lookups filter rows by scope inside the kernel
        default_ttl_s: Optional[float] = None,  # None: rows never expire
        _clock=time.monotonic,
    ):
        self.hip = _hip if _hip is not None else load_hip_module()
        if self.hip is None:
            raise RuntimeError("aigw_hip extension unavailable")
        self.device = torch.device(device)
        self.dim = dim
        self.capacity = capacity
        self.threshold = threshold
        g = torch.Generator().manual_seed(seed)
        # random-init bge-small-shaped weights (no network for checkpoints;
        # BASELINE.json: "synthetic OpenAI-schema payloads with random-init
        # embedding weights")
        self.emb = (
            torch.randn(vocab_size, dim, generator=g).to(torch.bfloat16).to(self.device)
        )
        self.proj = (
            (torch.randn(dim, dim, generator=g) / dim**0.5)
            .to(torch.bfloat16)
            .to(self.device)
        )
        self.index_dtype = (
            torch.float8_e4m3fn if index_dtype == "fp8" else torch.bfloat16
        )
        self.index = torch.zeros(capacity, dim, dtype=self.index_dtype, device=self.device)
        # per-row tag read by the scoped lookup kernel (12 B/row): scope id
        # and expiry in whole seconds of the cache's own clock, which
        # starts at 0 when the cache is built
        self.scoped = scoped
        self.default_ttl_s = default_ttl_s
        self.row_scope = torch.zeros(capacity, dtype=torch.int64, device=self.device)
        self.row_expiry = torch.zeros(capacity, dtype=torch.int32, device=self.device)
        self._clock = _clock
        self._t0 = _clock()
        # False until anything needs the tags; lookups stay on the
        # unfiltered kernel until then
        self._filtering = scoped or default_ttl_s is not None
        self.size = 0
        self.head = 0
        self.values: dict[int, bytes] = {}  # slot -> cached response body
        # inserts not yet all-gathered to the other shards (aigw.parallel)
        # as (vec, response, scope, expiry)
        self.pending: list[tuple[torch.Tensor, bytes, int, int]] = []
        self.record_pending = False

    def embed(self, out_ids: torch.Tensor, req_off: torch.Tensor) -> torch.Tensor:
        """(B, dim) bf16 L2-normalized query vectors from tokenizer output."""
        pooled = self.hip.meanpool(out_ids, req_off, self.emb)  # fp32 (B, dim)
        pooled_bf = pooled.to(torch.bfloat16)
        proj = self.hip.gemm_bf16_nt(pooled_bf, self.proj, None, False)  # fp32
        return self.hip.l2norm_rows(proj)

    def _now_f(self) -> float:
        return self._clock() - self._t0

    def now(self) -> int:
        """Whole seconds since the cache was built, clamped into
        [0, NEVER - 1]: it never wraps and a NEVER row never expires."""
        return int(min(max(self._now_f(), 0.0), NEVER - 1))

    def _expiry(self, ttl_s: Optional[float]) -> int:
        if ttl_s is None:
            ttl_s = self.default_ttl_s
        if ttl_s is None or ttl_s == math.inf:
            return NEVER
        if not ttl_s > 0:  # zero, negative or NaN: dead on arrival
            return 0
        # a row is live while expiry > now(); fractional ends round up
        return int(min(max(math.ceil(self._now_f() + ttl_s), 0.0), NEVER - 1))

    def lookup(
        self, queries: torch.Tensor, scopes: Optional[list[int]] = None
    ) -> list[Optional[tuple[int, float]]]:
        """Per query: (slot, score) of the best index row, or None.

        With ``scopes`` (one id per query, 0 = any scope), a scoped cache
        or any TTL in play, only live rows of the query's scope compete;
        otherwise every row does, as before the index had tags."""
        if self.size == 0:
            return [None] * queries.shape[0]
        view = self.index[: self.size]
        filtering = self._filtering or scopes is not None
        if filtering:
            n = queries.shape[0]
            q_scope = torch.tensor(
                list(scopes) if scopes is not None else [0] * n,
                dtype=torch.int64, device=self.device,
            )
            if q_scope.shape[0] != n:
                raise ValueError("scopes must hold one id per query")
            row_scope = self.row_scope[: self.size]
            row_expiry = self.row_expiry[: self.size]
            now = self.now()
        hi, idx = [], []
        for q0 in range(0, queries.shape[0], 256):  # kernel cap: 256 q/call
            qs = queries[q0 : q0 + 256].to(self.index_dtype).contiguous()
            if filtering:
                h, i = self.hip.cache_topk_scoped(
                    view, qs, row_scope, row_expiry, q_scope[q0 : q0 + 256], now
                )
            else:
                h, i = self.hip.cache_topk(view, qs)
            hi.extend(h.cpu().tolist())
            idx.extend(i.cpu().tolist())
        out = []
        for h, i in zip(hi, idx):
            if i < 0:  # scoped lookup: no row this query may see
                out.append(None)
                continue
            score = _unorder(h)
            out.append((i, score) if score >= self.threshold else None)
        return out

    def get(self, slot: int) -> Optional[bytes]:
        return self.values.get(slot)

    def _write_row(self, vec: torch.Tensor, response: bytes, scope: int,
                   expiry: int) -> int:
        slot = self.head
        self.index[slot] = vec
        self.row_scope[slot] = scope
        self.row_expiry[slot] = expiry
        self.values[slot] = response
        self.head = (self.head + 1) % self.capacity
        self.size = min(self.size + 1, self.capacity)
        if scope != 0 or expiry != NEVER:
            self._filtering = True
        return slot

    def insert(self, query_vec: torch.Tensor, response: bytes, scope: int = 0,
               ttl_s: Optional[float] = None) -> int:
        """Write the row and its tag into the ring (an overwritten slot
        loses its old tag with its old row). ``ttl_s=None`` takes the
        cache's default TTL, ``math.inf`` never expires, and a TTL that is
        not positive stores a row no lookup returns."""
        expiry = self._expiry(ttl_s)
        slot = self._write_row(query_vec.to(self.index_dtype), response, scope, expiry)
        if self.record_pending:
            self.pending.append((query_vec.detach(), response, scope, expiry))
        return slot

    def insert_remote(self, query_vec: torch.Tensor, response: bytes, scope: int = 0,
                      ttl_s: Optional[float] = None) -> int:
        """Insert a row replicated from another shard (never re-pended)."""
        return self._write_row(
            query_vec.to(self.index.dtype).to(self.device), response, scope,
            self._expiry(ttl_s),
        )

    def invalidate(self, scope: Optional[int] = None) -> int:
        """Set the expiry of every row of one scope (all rows for None) to
        0, drop their values, and drop the matching rows still queued for
        the other shards. Returns how many index rows it changed: every
        matching row not already invalidated, so rows whose TTL had run out
        count too. This shard only: rows already replicated stay live on
        the other shards."""
        self.pending = [p for p in self.pending
                        if scope is not None and p[2] != scope]
        if self.size == 0:
            return 0
        expiry = self.row_expiry[: self.size]
        hit = expiry != 0
        if scope is not None:
            hit &= self.row_scope[: self.size] == scope
        slots = torch.nonzero(hit).flatten()
        if slots.numel():
            expiry[slots] = 0
            self._filtering = True
            for s in slots.cpu().tolist():
                self.values.pop(s, None)
        return int(slots.numel())

    def _drain(self, max_n: int):
        batch, self.pending = self.pending[:max_n], self.pending[max_n:]
        if not batch:
            vecs = torch.zeros(0, self.dim, dtype=torch.bfloat16, device=self.device)
        else:
            vecs = torch.stack([b[0] for b in batch]).to(torch.bfloat16)
        return vecs, batch

    def drain_pending(self, max_n: int = 32):
        """Take up to max_n locally inserted rows for the next all-gather
        tick: returns (vecs [k, dim] on device, [response bytes])."""
        vecs, batch = self._drain(max_n)
        return vecs, [b[1] for b in batch]

    def drain_pending_scoped(self, max_n: int = 32):
        """drain_pending plus each row's tag for the receiving shards:
        (vecs, [response bytes], [(scope_id, ttl_remaining_s)]), the TTL in
        whole seconds from now (0 once it has run out), -1 for a row that
        never expires."""
        vecs, batch = self._drain(max_n)
        now = self.now()
        metas = [(b[2], -1 if b[3] == NEVER else max(b[3] - now, 0)) for b in batch]
        return vecs, [b[1] for b in batch], metas


def _unorder(u: int) -> float:
    """Reverse of pack_score's orderable-float transform (hi 32 bits)."""
    import struct

    u &= 0xFFFFFFFF
    bits = (u ^ 0x80000000) if u >= 0x80000000 else (~u & 0xFFFFFFFF)
    return struct.unpack("<f", struct.pack("<I", bits))[0]
