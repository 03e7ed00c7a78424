"""Semantic response cache: MFMA embedding + HBM-resident cosine index.

The embedding pipeline (mean-pooled token embeddings → bf16 MFMA projection
→ L2 normalize) runs entirely on the GPU from the tokenizer's on-device
output. The index is a ring buffer of bf16 rows sized for the 288 GB HBM3E
budget; lookup is the fused MFMA similarity + argmax kernel (one pass over
the index, no materialized score matrix).

Index rows are 128..512 wide (the arg-max kernels, every index dtype) or a
multiple of 128 up to 2048 (cache_topk_wide for bf16 and fp8 indexes, its
one-pass sibling cache_topk_wide_tiled for the batches that measured faster,
cache_topk_mxfp4_wide for mxfp4: 768, 1024, 1536 and 2048 are the widths of
the common embedding models). An mxfp4 index takes multiples of 128 only.
"""

from __future__ import annotations

import hashlib
import math
import time
from typing import Optional

import torch

from aigw.ops import load_hip_module


NEVER = 0x7FFFFFFF  # row_expiry of a row without a TTL

INDEX_DTYPES = {"bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn, "mxfp4": torch.uint8}

NARROW_MAX_DIM = 512  # widest row of cache_topk, cache_topk_scoped and cache_topk_k
WIDE_MAX_DIM = 2048  # widest row of cache_topk_wide


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
        # | "mxfp4" (OCP MX e2m1 blocks against fp8 queries: 208 B per
        # dim-384 row, 548 B per dim-1024 row, 3.7x the rows of bf16; dim a
        # multiple of 128 in 128..2048; aigw/ops/mxfp4_ref.py)
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
        if index_dtype not in INDEX_DTYPES:
            raise ValueError(
                f"index_dtype must be one of {', '.join(INDEX_DTYPES)}, got {index_dtype!r}")
        self.mxfp4 = index_dtype == "mxfp4"
        # rows past 512 elements are looked up by cache_topk_wide, or by
        # cache_topk_mxfp4_wide in an mxfp4 index
        self.wide = dim > NARROW_MAX_DIM
        if self.wide and not self.mxfp4 and (dim % 128 or dim > WIDE_MAX_DIM):
            raise ValueError(
                f"dim above {NARROW_MAX_DIM} must be a multiple of 128, at most "
                f"{WIDE_MAX_DIM}, got {dim}")
        # dtype of the stored rows; mxfp4 rows are packed nibbles
        self.index_dtype = INDEX_DTYPES[index_dtype]
        # dtype the lookup kernels take queries in
        self.query_dtype = torch.float8_e4m3fn if self.mxfp4 else self.index_dtype
        if self.mxfp4:
            if dim % 128 or not 128 <= dim <= WIDE_MAX_DIM:
                raise ValueError(
                    f"index_dtype='mxfp4' needs dim a multiple of 128 in "
                    f"128..{WIDE_MAX_DIM}, got {dim}")
            self.index = torch.zeros(capacity, dim // 2, dtype=torch.uint8, device=self.device)
            # one E8M0 scale byte per 32 elements, and 1/|dequantised row|
            self.index_scale = torch.full((capacity, dim // 32), 127, dtype=torch.uint8,
                                          device=self.device)
            self.index_inv_norm = torch.zeros(capacity, dtype=torch.float32,
                                              device=self.device)
        else:
            self.index = torch.zeros(capacity, dim, dtype=self.index_dtype,
                                     device=self.device)
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
        """(B, dim) bf16 L2-normalized query vectors from tokenizer output.

        The built-in embedder stops at dim 1024 (meanpool's limit); a cache
        with wider rows takes its callers' own vectors in ``insert`` and
        ``lookup``."""
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

    def _filter_tags(self, n: int, scopes: Optional[list[int]]):
        """(row_scope, row_expiry, q_scope, now) for a lookup of n queries
        that filters rows, None for one that does not: no ``scopes``, an
        unscoped cache and no TTL in play. q_scope covers all n queries; a
        call of at most 256 takes its slice."""
        if not self._filtering and scopes is None:
            return None
        q_scope = torch.tensor(
            list(scopes) if scopes is not None else [0] * n,
            dtype=torch.int64, device=self.device,
        )
        if q_scope.shape[0] != n:
            raise ValueError("scopes must hold one id per query")
        return self.row_scope[: self.size], self.row_expiry[: self.size], q_scope, self.now()

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
        filter_tags = self._filter_tags(queries.shape[0], scopes)
        filtering = filter_tags is not None
        if filtering:
            row_scope, row_expiry, q_scope, now = filter_tags
        hi, idx = [], []
        for q0 in range(0, queries.shape[0], 256):  # kernel cap: 256 q/call
            qs = queries[q0 : q0 + 256].to(self.query_dtype).contiguous()
            if self.mxfp4:
                rows = (view, self.index_scale[: self.size], self.index_inv_norm[: self.size])
                if self.wide:
                    tags = ((row_scope, row_expiry, q_scope[q0 : q0 + 256], now)
                            if filtering else ())
                    h, i = self.hip.cache_topk_mxfp4_wide(*rows, qs, *tags)
                elif filtering:
                    h, i = self.hip.cache_topk_mxfp4_scoped(
                        *rows, qs, row_scope, row_expiry, q_scope[q0 : q0 + 256], now
                    )
                else:
                    h, i = self.hip.cache_topk_mxfp4(*rows, qs)
            elif self.wide:
                tags = (row_scope, row_expiry, q_scope[q0 : q0 + 256], now) if filtering else ()
                if self._wide_tiled_serves(qs.shape[0], filtering):
                    h, i = self.hip.cache_topk_wide_tiled(view, qs, *tags)
                else:
                    h, i = self.hip.cache_topk_wide(view, qs, *tags)
            elif filtering:
                h, i = self.hip.cache_topk_scoped(
                    view, qs, row_scope, row_expiry, q_scope[q0 : q0 + 256], now
                )
            else:
                h, i = self.hip.cache_topk(view, qs)
            hi.extend(h.cpu().tolist())
            idx.extend(i.cpu().tolist())
        out = []
        for h, i in zip(hi, idx):
            if i < 0:  # scoped or wide lookup: no row this query may see
                out.append(None)
                continue
            score = _unorder(h)
            out.append((i, score) if score >= self.threshold else None)
        return out

    def _wide_pass(self, filtering: bool) -> int:
        """Queries one index pass of cache_topk_wide holds at this width."""
        return self.hip.cache_wide_queries_per_pass(
            self.dim, self.index_dtype == torch.float8_e4m3fn, filtering)

    def _wide_tiled_serves(self, n_q: int, filtering: bool) -> bool:
        """Whether cache_topk_wide_tiled (one index pass for any batch)
        takes a slice of n_q queries instead of cache_topk_wide (one pass
        per LDS-full of full-width queries). Only where it measured faster
        by more than 3% in both sweeps at 1M rows, the bold rows of
        profiles/cache_topk_wide_tiled.md. bf16: from 2 passes at dim >=
        1536; below that only filtered, from 3 passes. fp8: at dim >= 1536
        from 3 passes, and filtered at dim 1536 from 2. Everywhere else the
        multi-pass kernel is level or faster. Measured were dim 768 / 1024
        / 1536 / 2048 with 37 / 128 / 256 queries; the widths and pass
        counts between them follow the next lower measured one, by
        extrapolation, not measurement."""
        passes = -(-n_q // self._wide_pass(filtering))
        if self.index_dtype == torch.float8_e4m3fn:
            if self.dim < 1536:
                return False
            return passes >= 3 or (filtering and self.dim < 2048 and passes == 2)
        if self.dim >= 1536:
            return passes >= 2
        return filtering and passes >= 3

    def lookup_k(
        self, queries: torch.Tensor, k: int, scopes: Optional[list[int]] = None
    ) -> list[list[tuple[int, float]]]:
        """Per query: the at most k best index rows as (slot, score), best
        first (the higher slot first among equal scores), keeping only
        scores at or over the threshold. Rows are filtered exactly when
        ``lookup`` would filter them. One fused pass over the index
        (cache_topk_k); bf16 and fp8 indexes only.

        The first pair is not always what ``lookup`` returns: while no tag is
        in play ``lookup`` runs the unfiltered arg-max kernel, which gives an
        exact score tie between two rows of one aligned group of four slots
        (the same vector inserted back to back at slots 4m and 4m + 1) to the
        lower slot; ``lookup_k`` lists the higher slot first everywhere."""
        if self.mxfp4:
            raise ValueError(
                "lookup_k: k-best lookup is not implemented for index_dtype='mxfp4' "
                "(bf16 and fp8 only)")
        if self.wide:
            raise ValueError(
                f"lookup_k: k-best lookup serves dim <= {NARROW_MAX_DIM}, this cache "
                f"has dim {self.dim}")
        n = queries.shape[0]
        if self.size == 0:
            return [[] for _ in range(n)]
        view = self.index[: self.size]
        filter_tags = self._filter_tags(n, scopes)
        if filter_tags is not None:
            row_scope, row_expiry, q_scope, now = filter_tags
        out: list[list[tuple[int, float]]] = []
        for q0 in range(0, n, 256):  # kernel cap: 256 q/call
            qs = queries[q0 : q0 + 256].to(self.query_dtype).contiguous()
            if filter_tags is not None:
                h, i = self.hip.cache_topk_k(view, qs, k, row_scope, row_expiry,
                                             q_scope[q0 : q0 + 256], now)
            else:
                h, i = self.hip.cache_topk_k(view, qs, k)
            for hs, rows in zip(h.cpu().tolist(), i.cpu().tolist()):
                found = [(r, _unorder(x)) for x, r in zip(hs, rows) if r >= 0]
                out.append([(r, s) for r, s in found if s >= self.threshold])
        return out

    def get(self, slot: int) -> Optional[bytes]:
        return self.values.get(slot)

    def _write_row(self, vec: torch.Tensor, response: bytes, scope: int,
                   expiry: int) -> int:
        slot = self.head
        if self.mxfp4:
            packed, scale, inv_norm = self.hip.mxfp4_quantize_rows(
                vec.to(self.device, torch.bfloat16).reshape(1, self.dim))
            self.index[slot] = packed[0]
            self.index_scale[slot] = scale[0]
            self.index_inv_norm[slot] = inv_norm[0]
        else:
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
        vec = query_vec if self.mxfp4 else query_vec.to(self.index_dtype)
        slot = self._write_row(vec, response, scope, expiry)
        if self.record_pending:
            self.pending.append((query_vec.detach(), response, scope, expiry))
        return slot

    def insert_remote(self, query_vec: torch.Tensor, response: bytes, scope: int = 0,
                      ttl_s: Optional[float] = None) -> int:
        """Insert a row replicated from another shard (never re-pended)."""
        # an mxfp4 index quantises the replicated bf16 vector in _write_row
        vec = query_vec if self.mxfp4 else query_vec.to(self.index.dtype)
        return self._write_row(vec.to(self.device), response, scope, self._expiry(ttl_s))

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
