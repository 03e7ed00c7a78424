"""Index-scoped semantic cache, the CPU side: the gateway hands its scope
tag to GPU facades that advertise ``cache_scoped``, the UDS protocol and the
cross-shard sync carry it, and the CLI wires the flags. The kernel itself is
covered by tests/test_gpu_cache_scoped.py."""

import asyncio
import json
import multiprocessing as mp
import os
import struct
import tempfile

import pytest
import torch
import yaml

from aigw.extproc.lean_front import serve_lean
from aigw.extproc.server import GatewayServer, _cache_fingerprint
from aigw.extproc.upstream_client import LeanClient
from aigw.filterapi.config import RateLimitRule, load_config
from aigw.filterapi.runtime import RuntimeConfig
from aigw.ratelimit import RateLimiter


# ---- gateway -----------------------------------------------------------------


async def _start_counting_upstream():
    """OpenAI-shaped upstream whose n-th answer says "answer-n", so a served
    body names the request that produced it."""
    served = [0]

    async def handle(reader, writer):
        try:
            while True:
                head = await reader.readuntil(b"\r\n\r\n")
                n = 0
                for line in head.split(b"\r\n"):
                    if line.lower().startswith(b"content-length:"):
                        n = int(line.split(b":")[1])
                await reader.readexactly(n)
                served[0] += 1
                body = json.dumps({
                    "id": "c", "object": "chat.completion", "model": "m",
                    "choices": [{"index": 0, "finish_reason": "stop",
                                 "message": {"role": "assistant",
                                             "content": f"answer-{served[0]}"}}],
                    "usage": {"prompt_tokens": 1, "completion_tokens": 1,
                              "total_tokens": 2},
                }).encode()
                writer.write(b"HTTP/1.1 200 OK\r\ncontent-type: application/json\r\n"
                             b"content-length: %d\r\n\r\n" % len(body) + body)
                await writer.drain()
        except (asyncio.IncompleteReadError, ConnectionResetError):
            pass
        finally:
            writer.close()

    srv = await asyncio.start_server(handle, "127.0.0.1", 0)
    return srv, srv.sockets[0].getsockname()[1], served


def _cfg(up_port):
    return load_config(yaml.safe_load(f"""
routes:
  - name: r
    backends:
      - name: b
        schema: OpenAI
        upstream: {{host: 127.0.0.1, port: {up_port}}}
"""))


async def _gateway(gpu, with_fallback=False):
    up_srv, up_port, served = await _start_counting_upstream()
    server = GatewayServer(RuntimeConfig(_cfg(up_port)))
    server.gpu = gpu
    _, port, cleanup = await serve_lean(server, "127.0.0.1", 0,
                                        with_fallback=with_fallback)
    client = LeanClient()

    async def chat(auth, method_path="/v1/chat/completions", body=None):
        if body is None:
            body = {"model": "m", "messages": [{"role": "user", "content": "same text"}]}
        r = await client.post(
            host="127.0.0.1", port=port, tls=False, path=method_path,
            headers={"content-type": "application/json", "authorization": auth},
            body=json.dumps(body).encode(),
        )
        data = await r.read()
        hit = r.headers.get("x-aigw-cache") == "hit"
        status = r.status
        r.release()
        return status, hit, data

    async def close():
        await client.close()
        await cleanup()
        up_srv.close()

    return chat, close, served


class RecordingGPU:
    """Never hits; records the keyword arguments of every cache call."""

    cache_enabled = True

    def __init__(self, scoped):
        if scoped is not None:
            self.cache_scoped = scoped
        self.lookups, self.inserts = [], []

    async def cache_lookup_text(self, text, **kw):
        self.lookups.append(kw)
        return None, b"KEYVEC"

    async def cache_insert(self, vec, response, **kw):
        self.inserts.append(kw)

    async def count_text_tokens(self, text):
        return 0


@pytest.mark.parametrize("scoped", [None, False, True])
def test_scope_passed_only_to_scoped_facade(scoped):
    async def run():
        gpu = RecordingGPU(scoped)
        chat, close, _ = await _gateway(gpu)
        status, hit, data = await chat("Bearer user-a")
        assert status == 200 and not hit, data
        await close()
        return gpu

    gpu = asyncio.run(run())
    assert len(gpu.lookups) == 1 and len(gpu.inserts) == 1
    if scoped:
        body = {"model": "m", "messages": [{"role": "user", "content": "same text"}]}
        tag = b"U" + _cache_fingerprint("m", "r", body, {"authorization": "Bearer user-a"})
        assert gpu.lookups == [{"scope": tag}] and gpu.inserts == [{"scope": tag}]
    else:
        assert gpu.lookups == [{}] and gpu.inserts == [{}]


class ScopedIndexGPU:
    """Worst-case embedding (every text collides) over a multi-slot index
    that, like the scoped kernel, returns the newest row the scope may see."""

    cache_enabled = True
    cache_scoped = True

    def __init__(self):
        self.rows = []  # (scope, response)

    async def cache_lookup_text(self, text, scope=None):
        for s, resp in reversed(self.rows):
            if scope is None or s == scope:
                return resp, b"KEYVEC"
        return None, b"KEYVEC"

    async def cache_insert(self, vec, response, scope=None, ttl_s=None):
        self.rows.append((scope, response))

    async def cache_invalidate(self, scope=None):
        keep = [r for r in self.rows if scope is not None and r[0] != scope]
        n, self.rows = len(self.rows) - len(keep), keep
        return n

    async def count_text_tokens(self, text):
        return 0


def test_two_credentials_same_text_both_hit():
    async def run():
        gpu = ScopedIndexGPU()
        chat, close, served = await _gateway(gpu)
        sa, hit_a1, body_a1 = await chat("Bearer user-a")
        sb, hit_b1, body_b1 = await chat("Bearer user-b")
        assert (sa, sb) == (200, 200)
        assert not hit_a1 and not hit_b1 and served[0] == 2
        assert b"answer-1" in body_a1 and b"answer-2" in body_b1
        # second round: each credential finds its own row although b's row
        # is the newer one with the same key vector
        _, hit_a2, body_a2 = await chat("Bearer user-a")
        _, hit_b2, body_b2 = await chat("Bearer user-b")
        assert hit_a2 and hit_b2 and served[0] == 2
        assert body_a2 == body_a1 and body_b2 == body_b1
        assert b"answer-2" not in body_a2 and b"answer-1" not in body_b2

        # admin invalidation of one scope: a misses again, b still hits
        tag_a = gpu.rows[0][0]
        st, _, out = await chat("x", "/debug/cache/invalidate", {"scope": tag_a.hex()})
        assert st == 200 and json.loads(out) == {"invalidated": 1}, out
        _, hit_a3, _ = await chat("Bearer user-a")
        _, hit_b3, _ = await chat("Bearer user-b")
        assert not hit_a3 and hit_b3
        st, _, out = await chat("x", "/debug/cache/invalidate", {"scope": "zz"})
        assert st == 400, out
        await close()

    asyncio.run(run())


def test_invalidate_not_reachable_through_loopback_fallback():
    """With the loopback fallback app on (the CLI's default front), any
    spelling of the admin path that the lean front does not serve itself is
    relayed from 127.0.0.1. It must not reach the handler there: its
    loopback-only guard could not tell the relay from an operator."""
    async def run():
        gpu = ScopedIndexGPU()
        chat, close, _ = await _gateway(gpu, with_fallback=True)
        await chat("Bearer user-a")
        await chat("Bearer user-b")
        assert len(gpu.rows) == 2
        for target in ("/debug/cache/invalidate?x=1",
                       "/debug/cache/%69nvalidate",
                       "/debug/cache/invalidate/",
                       "//debug/cache/invalidate",
                       "/debug/cache/../cache/invalidate"):
            st, _, out = await chat("x", target, {})
            assert st in (404, 405), (target, st, out)
            assert len(gpu.rows) == 2, target
        # the exact path is served by the lean front, with the real peer
        st, _, out = await chat("x", "/debug/cache/invalidate", {})
        assert st == 200 and json.loads(out) == {"invalidated": 2}, out
        assert gpu.rows == []
        await close()

    asyncio.run(run())


def test_aiohttp_app_registers_invalidate_unless_switched_off():
    server = GatewayServer(RuntimeConfig(_cfg(1)))
    assert server.cache_invalidate_endpoint is True

    def paths(app):
        return {r.resource.canonical for r in app.router.routes()}

    assert "/debug/cache/invalidate" in paths(server.make_app())
    server.cache_invalidate_endpoint = False
    assert "/debug/cache/invalidate" not in paths(server.make_app())


# ---- SemanticCache host logic (CPU tensors; no kernel is reached) -------------


def _cpu_cache(clock, **kw):
    from aigw.ops.semcache import SemanticCache

    return SemanticCache(16, dim=8, capacity=8, device="cpu", _hip=object(),
                         _clock=clock, **kw)


def test_ttl_edges_and_scoped_drain():
    import math

    from aigw.ops.semcache import NEVER

    t = [0.0]
    cache = _cpu_cache(lambda: t[0], scoped=True)
    cache.record_pending = True
    v = torch.ones(8)
    cache.insert(v, b"never", scope=5)
    cache.insert(v, b"inf", scope=5, ttl_s=math.inf)
    cache.insert(v, b"zero", scope=5, ttl_s=0)
    cache.insert(v, b"neg", scope=5, ttl_s=-3)
    cache.insert(v, b"short", scope=6, ttl_s=2)
    cache.insert(v, b"long", scope=6, ttl_s=100.5)
    assert cache.row_expiry[:6].tolist() == [NEVER, NEVER, 0, 0, 2, 101]
    # drained 3 s later: the short row ran out a second ago; that is 0
    # ("drop it"), never the -1 that means "never expires"
    t[0] = 3.0
    _, values, metas = cache.drain_pending_scoped(32)
    assert values == [b"never", b"inf", b"zero", b"neg", b"short", b"long"]
    assert metas == [(5, -1), (5, -1), (5, 0), (5, 0), (6, 0), (6, 98)]


def test_invalidate_counts_rows_and_drops_pending():
    t = [0.0]
    cache = _cpu_cache(lambda: t[0], scoped=True)
    cache.record_pending = True
    v = torch.ones(8)
    cache.insert(v, b"a1", scope=1)
    cache.insert(v, b"a2", scope=1, ttl_s=5)
    cache.insert(v, b"b1", scope=2)
    t[0] = 10.0  # a2 has run out but was never invalidated: still counted
    assert cache.invalidate(scope=1) == 2
    assert cache.invalidate(scope=1) == 0
    assert cache.row_expiry[:3].tolist()[:2] == [0, 0]
    assert cache.values == {2: b"b1"}
    # rows of the scope still queued for the other shards go with it
    assert [p[1] for p in cache.pending] == [b"b1"]
    assert cache.invalidate() == 1
    assert cache.pending == [] and cache.values == {}


# ---- scope ids ---------------------------------------------------------------


def test_scope_id_stable_nonzero_int64(monkeypatch):
    import aigw.ops.semcache as sc

    assert sc.scope_id(b"x") == 4949498559009812781  # fixed across processes
    assert sc.SemanticCache.scope_id(b"x") == sc.scope_id(b"x")
    ids = {sc.scope_id(b"tenant-%d" % i) for i in range(2000)}
    assert len(ids) == 2000
    assert all(i != 0 and -(2**63) <= i < 2**63 for i in ids)
    assert any(i < 0 for i in ids)  # signed: the whole int64 range is used
    torch.tensor(sorted(ids), dtype=torch.int64)  # representable

    class Zero:
        def digest(self):
            return b"\0" * 32

    monkeypatch.setattr(sc.hashlib, "sha256", lambda b: Zero())
    assert sc.scope_id(b"anything") == 1  # 0 is the lookup wildcard


# ---- UDS protocol --------------------------------------------------------------


class FakeServices:
    """GPUServices stand-in behind GPUServiceHost; strict signatures, so a
    message without the optional fields must arrive without the kwargs."""

    def __init__(self):
        self.calls = []

    async def lookup_texts_batch(self, texts, scopes="absent"):
        self.calls.append(("lookup", list(texts), scopes))
        return [(None, f"vec-{t.decode()}") for t in texts]

    async def cache_insert(self, vec, response, scope="absent", ttl_s="absent"):
        self.calls.append(("insert", vec, response, scope, ttl_s))

    async def cache_invalidate(self, scope=None):
        self.calls.append(("invalidate", scope))
        return 3


def test_uds_messages_round_trip_scopes():
    from aigw.gpu.service import GPUServiceHost, RemoteGPUClient

    async def run():
        gpu = FakeServices()
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "gpu.sock")
            host = GPUServiceHost(gpu, path)
            await host.start()
            client = RemoteGPUClient(path, enable_cache=True, cache_scoped=True)
            assert client.cache_scoped is True
            assert RemoteGPUClient(path).cache_scoped is False
            # one flush: a scoped and an unscoped text in the same batch
            (_, h1), (_, h2) = await asyncio.gather(
                client.cache_lookup_text(b"t1", scope=b"S\x00\xfftag"),
                client.cache_lookup_text(b"t2"),
            )
            await client.cache_insert(h1, b"resp1", scope=b"S\x00\xfftag", ttl_s=2.5)
            await client.cache_insert(h2, b"resp2")
            # no scope anywhere -> the message has no scopes field
            _, h3 = await client.cache_lookup_text(b"t3")
            assert await client.cache_invalidate(b"S\x00\xfftag") == 3
            client.close()
            await host.stop()
        return gpu.calls

    calls = asyncio.run(run())
    assert calls == [
        ("lookup", [b"t1", b"t2"], [b"S\x00\xfftag", None]),
        ("insert", "vec-t1", b"resp1", b"S\x00\xfftag", 2.5),
        ("insert", "vec-t2", b"resp2", "absent", "absent"),
        ("lookup", [b"t3"], "absent"),
        ("invalidate", b"S\x00\xfftag"),
    ]


# ---- CLI -----------------------------------------------------------------------


@pytest.mark.parametrize("flag", [["--semantic-cache-scope", "index"],
                                  ["--semantic-cache-ttl", "30"]])
def test_cli_rejects_index_scope_and_ttl_under_native_front(flag):
    from aigw.cli.main import main

    with pytest.raises(SystemExit) as e:
        main(["run", "--front", "fast", "--gpu", "--semantic-cache", *flag])
    assert "native front" in str(e.value) and "not supported" in str(e.value)


# ---- cross-shard replication -----------------------------------------------------


class ScopedFakeCache:
    """CPU stand-in with SemanticCache's scoped sync interface."""

    dim = 8
    scoped = True

    def __init__(self):
        self.device = torch.device("cpu")
        self.pending = []  # (vec, value, scope, ttl_remaining_s)
        self.remote = []  # (vec, value, scope, ttl_s)

    def drain_pending_scoped(self, max_n=32):
        batch, self.pending = self.pending[:max_n], self.pending[max_n:]
        if not batch:
            return torch.zeros(0, self.dim, dtype=torch.bfloat16), [], []
        return (torch.stack([b[0] for b in batch]).to(torch.bfloat16),
                [b[1] for b in batch], [(b[2], b[3]) for b in batch])

    def insert_remote(self, vec, value, scope=0, ttl_s=None):
        self.remote.append((vec, value, scope, ttl_s))


class PlainFakeCache:
    """The unscoped sync interface: no ``scoped`` attribute at all."""

    dim = 8

    def __init__(self):
        self.device = torch.device("cpu")
        self.pending = []  # (vec, value)

    def drain_pending(self, max_n=32):
        batch, self.pending = self.pending[:max_n], self.pending[max_n:]
        return (torch.stack([v for v, _ in batch]).to(torch.bfloat16),
                [r for _, r in batch])


def _scoped_sync_worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist

        from aigw.parallel import StateSync

        dist.init_process_group("gloo", rank=rank, world_size=world)
        limiter = RateLimiter(
            [RateLimitRule(name="b", metadata_key="llm_total_token", limit=10, window_s=60)]
        )
        cache = ScopedFakeCache()
        sync = StateSync(limiter, cache=cache)
        if rank == 0:
            cache.pending = [
                (torch.arange(8, dtype=torch.float32), b"ttl-row", -(2**63) + 5, 42),
                (torch.ones(8), b"expired-row", 7, 0),
                (torch.ones(8), b"long-expired-row", 7, -3),
                (torch.zeros(8), b"", 2**63 - 1, -1),  # empty body, never expires
            ]
        sync.tick_sync()
        sync.tick_sync()  # nothing pending: no-op collectives
        if rank == 1:
            got = [(v, s, t) for _vec, v, s, t in cache.remote]
            assert got == [(b"ttl-row", -(2**63) + 5, 42),
                           (b"", 2**63 - 1, None)], got
            assert torch.allclose(cache.remote[0][0].float(),
                                  torch.arange(8, dtype=torch.float32), atol=0.1)
        else:
            assert cache.remote == []
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback

        q.put((rank, f"FAIL: {e}\n{traceback.format_exc()}"))


def test_scoped_cache_sync_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_scoped_sync_worker, args=(r, 2, 29771, q))
             for r in range(2)]
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


class _RecordingDist:
    """Single-rank stand-in for torch.distributed inside _sync_cache."""

    def __init__(self):
        self.sent = []

    def get_rank(self, group=None):
        return 0

    def get_world_size(self, group=None):
        return 1

    def all_gather(self, out, t, group=None):
        self.sent.append(t.clone())
        out[0].copy_(t)


def _sync_payload(monkeypatch, cache):
    import aigw.parallel.state_sync as ss

    rec = _RecordingDist()
    monkeypatch.setattr(ss, "dist", rec)
    sync = ss.StateSync.__new__(ss.StateSync)
    sync.cache, sync.group, sync.device = cache, None, torch.device("cpu")
    sync._sync_cache()
    assert len(rec.sent) == 3  # sizes, vecs, payload
    sizes, vecs, payload = rec.sent
    return sizes.tolist(), vecs, bytes(payload.numpy().tobytes())


def test_sync_payload_bytes(monkeypatch):
    """Unscoped cache: the wire bytes of the format before row tags
    (4-byte length + body per record). Scoped: the same records, each with
    the 12-byte (int64 scope, int32 ttl) trailer."""
    values = [b"response-zero", b"", b"x" * 300]
    plain = PlainFakeCache()
    plain.pending = [(torch.full((8,), float(i)), v) for i, v in enumerate(values)]
    sizes, vecs, payload = _sync_payload(monkeypatch, plain)
    want = b"".join(len(v).to_bytes(4, "little") + v for v in values)
    assert sizes == [3, len(want)] and payload == want
    assert vecs.dtype == torch.bfloat16 and vecs.shape == (3, 8)

    scoped = ScopedFakeCache()
    metas = [(11, 30), (-4, -1), (2**62, 1)]
    scoped.pending = [(torch.full((8,), float(i)), v, *m)
                      for i, (v, m) in enumerate(zip(values, metas))]
    sizes, _, payload = _sync_payload(monkeypatch, scoped)
    want = b"".join(len(v).to_bytes(4, "little") + v + struct.pack("<qi", *m)
                    for v, m in zip(values, metas))
    assert sizes == [3, len(want)] and payload == want
