"""Async facade over the GPU ops for the gateway hot path.

Requests never launch kernels individually: a micro-batching collector
coalesces concurrent requests (up to ``max_batch`` or ``window_ms``) into
one packed tokenizer launch — the LDS-staged "batched 4k-token chat
payloads" admission model from BASELINE.json — and, for cache-enabled
requests, one embedding GEMM + one fused index lookup. GPU work runs on a
dedicated single-thread executor so kernel syncs never stall the event
loop.
"""

from __future__ import annotations

import asyncio
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Optional

import torch


def extract_chat_text(body: dict) -> bytes:
    """Concatenated message text of a chat request (OpenAI or Anthropic
    shape) — the tokenizer input for admission accounting."""
    parts: list[str] = []
    system = body.get("system")
    if isinstance(system, str):
        parts.append(system)
    for msg in body.get("messages") or []:
        c = msg.get("content")
        if isinstance(c, str):
            parts.append(c)
        elif isinstance(c, list):
            for p in c:
                if isinstance(p, dict):
                    t = p.get("text") or ""
                    if t:
                        parts.append(t)
    return "\n".join(parts).encode("utf-8", "replace")[:262144] or b" "


def _scope_id(scope) -> int:
    """Index scope id of a caller's scope: None is the wildcard 0, bytes
    (a scope tag) hash through SemanticCache.scope_id, ints pass."""
    if scope is None:
        return 0
    if isinstance(scope, int):
        return scope
    from aigw.ops.semcache import scope_id

    return scope_id(bytes(scope))


class PrefixPick(int):
    """Replica row picked by the prefix-cache-aware scorer: an int that
    also says how many of the prompt's tokens the replica had seen."""

    def __new__(cls, index: int, matched_tokens: int = 0, prompt_tokens: int = 0):
        self = super().__new__(cls, index)
        self.matched_tokens = int(matched_tokens)
        self.prompt_tokens = int(prompt_tokens)
        return self


@dataclass
class _Pending:
    """One queued work item: a BATCH of texts sharing a future (single
    requests are 1-element batches; the shard GPU service submits whole
    worker batches so the per-text future overhead disappears)."""

    texts: list
    want_vec: bool
    scopes: Optional[list] = None  # cache scope id per text (0 = any scope)
    future: asyncio.Future = None  # type: ignore[assignment]


class GPUServices:
    def __init__(
        self,
        device: str = "cuda",
        *,
        n_merges: int = 32768,
        enable_cache: bool = False,
        cache_capacity: int = 65536,
        cache_threshold: float = 0.92,
        cache_index_dtype: str = "bf16",  # "bf16" | "fp8" (2x rows/GB, faster lookups)
        cache_scoped: bool = False,  # filter cache rows by scope in the index
        cache_ttl_s: Optional[float] = None,  # None: cached rows never expire
        window_ms: float = 0.1,
        max_batch: int = 128,
    ):
        from aigw.ops.semcache import SemanticCache
        from aigw.ops.tokenizer import GPUTokenizer

        self.device = device
        self.tokenizer = GPUTokenizer(n_merges=n_merges, device=device)
        self.cache: Optional[SemanticCache] = (
            SemanticCache(
                self.tokenizer.vocab_size,
                capacity=cache_capacity,
                threshold=cache_threshold,
                device=device,
                index_dtype=cache_index_dtype,
                scoped=cache_scoped,
                default_ttl_s=cache_ttl_s,
            )
            if enable_cache
            else None
        )
        # advertised to GatewayServer: when set it passes each request's
        # scope tag to lookup and insert
        self.cache_scoped = cache_scoped
        self.window_ms = window_ms
        self.max_batch = max_batch
        import os as _os

        # Measured NEGATIVE (profiles/r01 ab.jsonl): the sync-free
        # event-polling count path is ~20% slower at 12 workers — executor
        # threads may freely spin on this many-core node, while 0.2 ms
        # event polling adds per-batch latency. Kept behind an opt-in for
        # core-constrained deployments.
        self.async_counts = _os.environ.get("AIGW_GPU_ASYNC_PATH", "") == "1"
        self._prefix: dict = {}  # pool name -> PrefixIndex, built lazily
        self.prefix_rows_dropped = 0  # replicated rows of pools not built here
        self._pending: list[_Pending] = []
        self._pending_texts = 0
        self._flush_handle = None
        self._executor = ThreadPoolExecutor(max_workers=1, thread_name_prefix="aigw-gpu")
        self._lock = asyncio.Lock()

    @property
    def cache_enabled(self) -> bool:
        return self.cache is not None

    # ---- batching core -------------------------------------------------------

    async def _submit_batch(self, texts: list, want_vec: bool, scopes=None):
        loop = asyncio.get_running_loop()
        item = _Pending(texts=texts, want_vec=want_vec, scopes=scopes,
                        future=loop.create_future())
        self._pending.append(item)
        self._pending_texts += len(texts)
        if self._pending_texts >= self.max_batch:
            if self._flush_handle:
                self._flush_handle.cancel()
                self._flush_handle = None
            asyncio.ensure_future(self._flush())
        elif self._flush_handle is None:
            self._flush_handle = loop.call_later(
                self.window_ms / 1000.0, lambda: asyncio.ensure_future(self._flush())
            )
        return await item.future

    async def _submit(self, text: bytes, want_vec: bool, scope=None):
        scopes = None if scope is None else [_scope_id(scope)]
        out = await self._submit_batch([text], want_vec, scopes)
        return out[0]  # (count, vec, cached_value)

    async def _flush(self):
        self._flush_handle = None
        batch, self._pending = self._pending, []
        self._pending_texts = 0
        if not batch:
            return
        loop = asyncio.get_running_loop()
        if self.async_counts and not any(it.want_vec for it in batch):
            # count-only fast path: launch without ANY host sync and await
            # the completion event cooperatively — a blocking torch sync on
            # ROCm busy-spins a core per worker, which halved 12-worker
            # serving throughput (profiles/r01)
            try:
                counts_gpu, spans = await loop.run_in_executor(
                    self._executor, self._launch_counts, batch
                )
                ev = counts_gpu["ev"]
                while not ev.query():
                    await asyncio.sleep(0.0002)
                counts_host = counts_gpu["counts"].cpu().tolist()
            except Exception as e:  # pragma: no cover - defensive
                for it in batch:
                    if not it.future.done():
                        it.future.set_exception(e)
                return
            for it, (lo, hi) in zip(batch, spans):
                if not it.future.done():
                    it.future.set_result(
                        [(counts_host[i], None, None) for i in range(lo, hi)]
                    )
            return
        try:
            results = await loop.run_in_executor(self._executor, self._run_batch, batch)
        except Exception as e:  # pragma: no cover - defensive
            for it in batch:
                if not it.future.done():
                    it.future.set_exception(e)
            return
        for it, res in zip(batch, results):
            if not it.future.done():
                it.future.set_result(res)

    def _launch_counts(self, batch: list[_Pending]):
        """GPU worker thread: pack + H2D + kernel launches, NO sync."""
        texts = []
        spans = []
        for it in batch:
            spans.append((len(texts), len(texts) + len(it.texts)))
            texts.extend(it.texts)
        counts_gpu, _ids, _off, ev = self.tokenizer.encode_batch_async(texts)
        return {"counts": counts_gpu, "ev": ev}, spans

    def _run_batch(self, batch: list[_Pending]):
        """Executed on the GPU worker thread: one packed tokenizer launch
        over every text of every queued batch; for vector-wanting items,
        ONE batched embedding GEMM and ONE fused index lookup (a lookup per
        request would mean a single-query kernel launch each). Returns one
        result list per item of (count, vec, cached_value_or_None)."""
        texts = []
        spans = []
        for it in batch:
            spans.append((len(texts), len(texts) + len(it.texts)))
            texts.extend(it.texts)
        counts, _, state = self.tokenizer.encode_batch(texts)
        counts_host = counts.cpu().tolist()
        qvecs = None
        hits = None
        if any(it.want_vec for it in batch) and self.cache is not None:
            qvecs = self.cache.embed(state["out_ids"], state["req_off"])
            scopes = None
            if any(it.scopes is not None for it in batch):
                # unscoped items ride the same lookup as wildcards
                scopes = []
                for it in batch:
                    scopes.extend(it.scopes if it.scopes is not None
                                  else [0] * len(it.texts))
            # one fused kernel, all queries
            found = self.cache.lookup(qvecs, scopes=scopes)
            hits = [self.cache.get(h[0]) if h is not None else None for h in found]
        results = []
        for it, (lo, hi) in zip(batch, spans):
            if it.want_vec and qvecs is not None:
                results.append(
                    [(counts_host[i], qvecs[i], hits[i]) for i in range(lo, hi)]
                )
            else:
                results.append([(counts_host[i], None, None) for i in range(lo, hi)])
        return results

    # ---- public API ----------------------------------------------------------

    async def count_request_tokens(self, body: dict) -> int:
        count, _, _ = await self._submit(extract_chat_text(body), want_vec=False)
        return count

    async def count_text_tokens(self, text: bytes) -> int:
        count, _, _ = await self._submit(text or b" ", want_vec=False)
        return count

    async def count_texts_batch(self, texts: list[bytes]) -> list[int]:
        """Batch entry used by the shard GPU service: one future per worker
        batch; texts from many workers coalesce into one kernel launch."""
        results = await self._submit_batch([t or b" " for t in texts], want_vec=False)
        return [r[0] for r in results]

    async def cache_lookup_text(self, text: bytes, scope=None):
        """Like cache_lookup but takes pre-extracted text (from the C++
        scanner) instead of a parsed body. Lookup is part of the batched
        flush — no per-request kernel launches. ``scope`` (a tag's bytes or
        an id) restricts the lookup to that scope's rows."""
        _, vec, hit = await self._submit(text or b" ", want_vec=True, scope=scope)
        return hit, vec

    async def lookup_texts_batch(self, texts: list[bytes], scopes=None):
        """Batch entry for the shard GPU service: one future per worker
        batch; returns [(hit_or_None, vec)] aligned with texts. ``scopes``
        holds one scope (bytes, id or None) per text."""
        if scopes is not None:
            if len(scopes) != len(texts):
                raise ValueError("scopes must align with texts")
            scopes = [_scope_id(s) for s in scopes]
        results = await self._submit_batch(
            [t or b" " for t in texts], want_vec=True, scopes=scopes
        )
        return [(hit, vec) for _c, vec, hit in results]

    async def tokenize(self, text) -> list[int]:
        if isinstance(text, str):
            text = text.encode("utf-8", "replace")
        loop = asyncio.get_running_loop()

        def run():
            _, ids, _ = self.tokenizer.encode_batch([text or b" "], return_ids=True)
            return ids[0]

        return await loop.run_in_executor(self._executor, run)

    async def cache_lookup(self, body: dict, scope=None):
        """Returns (cached_response_bytes | None, query_vec)."""
        _, vec, hit = await self._submit(
            extract_chat_text(body), want_vec=True, scope=scope
        )
        return hit, vec

    async def cache_insert(self, vec, response: bytes, scope=None, ttl_s=None) -> None:
        if vec is None or self.cache is None:
            return
        loop = asyncio.get_running_loop()
        await loop.run_in_executor(
            self._executor, self.cache.insert, vec, response, _scope_id(scope), ttl_s
        )

    async def cache_invalidate(self, scope=None) -> int:
        """Expire the cached rows of one scope (all rows for None)."""
        if self.cache is None:
            return 0
        loop = asyncio.get_running_loop()
        return await loop.run_in_executor(
            self._executor, self.cache.invalidate,
            None if scope is None else _scope_id(scope),
        )

    async def pick_endpoint(self, stats_rows: list[list[float]], predicted: float) -> int:
        """One KV-occupancy scoring call for a single request: returns the
        index of the replica to try first (InferencePool EPP analogue)."""
        loop = asyncio.get_running_loop()

        def run():
            stats = torch.tensor(stats_rows, dtype=torch.float32, device=self.device)
            pred = torch.tensor([predicted], dtype=torch.float32, device=self.device)
            hip = self.tokenizer.hip
            return int(hip.kv_score_assign(stats, pred, 1.0, 0.1, 0.05).cpu()[0])

        return await loop.run_in_executor(self._executor, run)

    # ---- prefix-cache-aware picking ------------------------------------------

    def _prefix_index(self, pool: str, settings: Optional[dict]):
        """The pool's PrefixIndex, built on first use from the route's
        prefixCache settings (GPU executor thread only)."""
        idx = self._prefix.get(pool)
        if idx is None:
            from aigw.ops.prefixindex import PrefixIndex

            s = settings or {}
            idx = PrefixIndex(
                pool,
                block_tokens=int(s.get("block_tokens", 16)),
                max_blocks=int(s.get("max_blocks", 256)),
                buckets=int(s.get("buckets", 65536)),
                ttl_s=s.get("ttl_s", 300.0),
                weight=float(s.get("weight", 1.0)),
                replicate=bool(s.get("replicate", False)),
                device=self.device,
                _hip=self.tokenizer.hip,
            )
            self._prefix[pool] = idx
        return idx

    def _assign_prefix(self, pool, members, stats, texts, predicted, settings):
        """GPU executor thread: tokenise (one packed, sync-free launch
        chain), hash, match, score, insert; ONE host sync at the end."""
        idx = self._prefix_index(pool, settings)
        texts = [t or b" " for t in texts]
        counts, out_ids, req_off, _ev = self.tokenizer.encode_batch_async(texts)
        if not torch.is_tensor(stats):
            stats = torch.tensor(stats, dtype=torch.float32)
        stats = stats.to(self.device, torch.float32).contiguous()
        if predicted is None:
            pred = counts.to(torch.float32)  # the prompts' own token counts
        else:
            if not torch.is_tensor(predicted):
                predicted = torch.tensor(list(predicted), dtype=torch.float32)
            pred = predicted.to(self.device, torch.float32).contiguous()
        assign, hit, _nb = idx.assign(
            members, stats, pred, out_ids, req_off, sum(len(t) for t in texts)
        )
        matched = torch.minimum(hit * idx.block_tokens, counts)
        host = torch.stack([assign, matched, counts]).cpu().tolist()  # the sync
        return [PrefixPick(a, m, c) for a, m, c in zip(*host)]

    async def assign_replicas_prefix(self, pool: str, members, stats, texts,
                                     predicted=None, settings: Optional[dict] = None):
        """Batched prefix-cache-aware assignment for one pool: texts[i]
        goes to replica row result[i] of ``stats`` (rows in ``members``
        order). ``predicted`` (tokens per request) defaults to the
        prompts' own token counts. Each result is a PrefixPick."""
        loop = asyncio.get_running_loop()
        return await loop.run_in_executor(
            self._executor, self._assign_prefix, pool, list(members), stats,
            list(texts), predicted, settings,
        )

    async def pick_endpoint_prefix(self, pool: str, members, stats_rows, text: bytes,
                                   predicted: float,
                                   settings: Optional[dict] = None) -> int:
        """pick_endpoint with the prefix-hit term: prefers the replica
        whose KV cache already holds the longest prefix of ``text``."""
        picks = await self.assign_replicas_prefix(
            pool, members, stats_rows, [text], [float(predicted)], settings
        )
        return picks[0]

    def prefix_stats(self) -> dict:
        return {pool: idx.stats() for pool, idx in self._prefix.items()}

    # ---- prefix index replication (driven by StateSync, which runs on its
    #      own thread: every index is touched on the GPU executor only) -------

    def prefix_prepare(self, pool: str, settings: Optional[dict] = None) -> None:
        """Build the pool's index now, not on its first pick, so that rows
        other shards send for it have somewhere to go from the start."""
        self._executor.submit(self._prefix_index, pool, settings).result()

    def _prefix_drain(self, max_n: int) -> torch.Tensor:
        parts, left = [], int(max_n)
        for idx in self._prefix.values():
            if not idx.replicate or left <= 0:
                continue
            rec = idx.drain_log(left)
            if rec.shape[0]:
                salt = torch.full((rec.shape[0], 1), idx.salt, dtype=torch.int64,
                                  device=rec.device)
                parts.append(torch.cat([rec, salt], dim=1))
                left -= rec.shape[0]
        if not parts:
            return torch.zeros(0, 3, dtype=torch.int64, device=self.device)
        return torch.cat(parts)

    def prefix_drain_sync(self, max_n: int) -> torch.Tensor:
        """Blocking: the oldest <= max_n replication records over all
        replicating pools, as int64[k, 3] rows of (hash, member key,
        salt_of(pool)) on the device."""
        return self._executor.submit(self._prefix_drain, max_n).result()

    def _prefix_apply(self, rows: torch.Tensor) -> None:
        rows = rows.to(self.device, torch.int64)
        if rows.shape[0] == 0:
            return
        by_salt = {idx.salt: idx for idx in self._prefix.values() if idx.replicate}
        done = 0
        for salt in torch.unique(rows[:, 2]).cpu().tolist():
            idx = by_salt.get(salt)
            if idx is None:
                continue
            rec = rows[rows[:, 2] == salt][:, :2].contiguous()  # keeps list order
            idx.apply_remote(rec)
            done += rec.shape[0]
        self.prefix_rows_dropped += rows.shape[0] - done

    def prefix_apply_sync(self, rows: torch.Tensor) -> None:
        """Blocking: apply another shard's drained rows, routed by salt.
        Rows of a pool that is not built (or not replicating) here are
        dropped and counted in ``prefix_rows_dropped``."""
        self._executor.submit(self._prefix_apply, rows).result()

    async def assign_replicas(self, stats: torch.Tensor, predicted: torch.Tensor):
        loop = asyncio.get_running_loop()
        hip = self.tokenizer.hip

        def run():
            return hip.kv_score_assign(stats, predicted, 1.0, 0.1, 0.05).cpu().tolist()

        return await loop.run_in_executor(self._executor, run)

    def close(self):
        self._executor.shutdown(wait=False)
