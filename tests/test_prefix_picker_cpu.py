"""prefixCache route option: config validation, the server's use of
pick_endpoint_prefix (fake GPU object, as tests/test_endpoint_picker.py),
the socket service's pick_prefix op and PrefixIndex's member-bit map."""

import asyncio
import os
import tempfile

import aiohttp
import pytest
import torch

from aigw.extproc.server import GatewayServer, run_server
from aigw.filterapi import RuntimeConfig, load_config
from aigw.filterapi.config import ConfigError, PrefixCache
from aigw.gpu.services import PrefixPick
from aigw.testing.mockupstream import start_mock_upstream

UP = {"host": "127.0.0.1", "port": 1}


def _cfg(prefix_cache=None, picker=True, up=UP):
    route = {
        "name": "pool",
        "backends": [
            {"name": f"replica-{i}", "schema": "OpenAI", "upstream": up,
             "headerMutation": {"set": {"x-replica": str(i)}}}
            for i in range(3)
        ],
    }
    if picker:
        route["endpointPicker"] = True
    if prefix_cache is not None:
        route["prefixCache"] = prefix_cache
    return {"version": "v1", "routes": [route]}


# ---- config ------------------------------------------------------------------


def test_prefix_cache_defaults_and_values():
    cfg = load_config(_cfg({}))
    assert cfg.routes[0].prefix_cache == PrefixCache(16, 256, 65536, 300.0, 1.0)
    cfg = load_config(_cfg({"blockTokens": 64, "maxBlocks": 32, "buckets": 1024,
                            "ttlS": 5, "weight": 0.5}))
    assert cfg.routes[0].prefix_cache == PrefixCache(64, 32, 1024, 5, 0.5)
    assert load_config(_cfg()).routes[0].prefix_cache is None


@pytest.mark.parametrize("bad", [
    {"blockTokens": 12}, {"blockTokens": 128}, {"blockTokens": "16"},
    {"buckets": 1000}, {"buckets": 0}, {"maxBlocks": 257}, {"maxBlocks": 0},
    {"ttlS": 0}, {"weight": -1}, {"blocks": 3},
])
def test_prefix_cache_rejects_bad_values(bad):
    with pytest.raises(ConfigError):
        load_config(_cfg(bad))


def test_prefix_cache_needs_the_endpoint_picker():
    with pytest.raises(ConfigError, match="endpointPicker"):
        load_config(_cfg({}, picker=False))


# ---- server ------------------------------------------------------------------


class FakeGPU:
    cache_enabled = False

    def __init__(self, pick=1, prefix_pick=2, fail=False):
        self.pick, self.prefix_pick, self.fail = pick, prefix_pick, fail
        self.plain_calls, self.prefix_calls = [], []

    async def count_request_tokens(self, body):
        return 100

    async def count_text_tokens(self, text):
        return 100

    async def pick_endpoint(self, stats_rows, predicted):
        self.plain_calls.append((stats_rows, predicted))
        return self.pick

    async def pick_endpoint_prefix(self, pool, members, stats_rows, text, predicted,
                                   settings=None):
        self.prefix_calls.append((pool, members, stats_rows, text, predicted, settings))
        if self.fail:
            raise RuntimeError("index unavailable")
        return PrefixPick(self.prefix_pick, 48, 100)

    async def tokenize(self, text):
        return [1]


def _serve(gpu, prefix_cache):
    async def main():
        mock, up_runner, up_port = await start_mock_upstream()
        mock.record = True
        cfg = load_config(_cfg(prefix_cache, up={"host": "127.0.0.1", "port": up_port}))
        server = GatewayServer(RuntimeConfig(cfg), gpu_services=gpu)
        gw = await run_server(server, host="127.0.0.1", port=0)
        port = gw.addresses[0][1]
        async with aiohttp.ClientSession() as client:
            async with client.post(
                f"http://127.0.0.1:{port}/v1/chat/completions",
                json={"model": "m", "messages": [
                    {"role": "system", "content": "be brief"},
                    {"role": "user", "content": "what is a wavefront?"}]},
            ) as r:
                assert r.status == 200
            async with client.get(f"http://127.0.0.1:{port}/metrics") as r:
                metrics = await r.text()
        replica = mock.requests[-1]["headers"]["x-replica"]
        await gw.cleanup()
        await up_runner.cleanup()
        return replica, metrics

    return asyncio.run(main())


def test_prefix_route_calls_the_prefix_pick_with_names_and_text():
    gpu = FakeGPU()
    replica, metrics = _serve(gpu, {"blockTokens": 8, "buckets": 256})
    assert replica == "2" and not gpu.plain_calls
    pool, members, stats_rows, text, predicted, settings = gpu.prefix_calls[0]
    assert pool == "pool" and members == ["replica-0", "replica-1", "replica-2"]
    assert len(stats_rows) == 3 and predicted == 100.0
    assert b"be brief" in text and b"what is a wavefront?" in text
    assert settings == {"block_tokens": 8, "max_blocks": 256, "buckets": 256,
                        "ttl_s": 300.0, "weight": 1.0}
    assert 'aigw_prefix_cache_matched_tokens_total{route="pool"} 48.0' in metrics
    assert 'aigw_prefix_cache_picked_tokens_total{route="pool"} 100.0' in metrics


def test_plain_picker_route_still_calls_pick_endpoint():
    gpu = FakeGPU()
    replica, _ = _serve(gpu, None)
    assert replica == "1" and len(gpu.plain_calls) == 1 and not gpu.prefix_calls


def test_prefix_pick_failure_falls_back_to_pick_endpoint():
    gpu = FakeGPU(fail=True)
    replica, _ = _serve(gpu, {})
    assert len(gpu.prefix_calls) == 1 and len(gpu.plain_calls) == 1
    assert replica == "1"


def test_out_of_range_prefix_pick_falls_back():
    gpu = FakeGPU(prefix_pick=7)
    replica, _ = _serve(gpu, {})
    assert replica == "1" and len(gpu.plain_calls) == 1


# ---- socket service ----------------------------------------------------------


def test_pick_prefix_op_round_trip():
    from aigw.gpu.service import GPUServiceHost, RemoteGPUClient

    async def main():
        gpu = FakeGPU(prefix_pick=2)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "gpu.sock")
            host = GPUServiceHost(gpu, path)
            await host.start()
            client = RemoteGPUClient(path)
            pick = await client.pick_endpoint_prefix(
                "pool", ["a", "b", "c"], [[0, 1, 0, 0]] * 3, b"hello", 12,
                settings={"block_tokens": 8})
            plain = await client.pick_endpoint([[0, 1, 0, 0]] * 3, 12)
            client.close()
            await host.stop()
        return pick, plain, gpu

    pick, plain, gpu = asyncio.run(main())
    assert pick == 2 and pick.matched_tokens == 48 and pick.prompt_tokens == 100
    assert plain == 1
    pool, members, stats_rows, text, predicted, settings = gpu.prefix_calls[0]
    assert (pool, members, text, predicted) == ("pool", ["a", "b", "c"], b"hello", 12.0)
    assert settings == {"block_tokens": 8} and len(stats_rows) == 3


# ---- PrefixIndex member bits ---------------------------------------------------


class FakeHip:
    def __init__(self):
        self.cleared = []

    def prefix_clear_bits(self, masks, mask):
        self.cleared.append(mask)


def _index(**kw):
    from aigw.ops.prefixindex import PrefixIndex

    hip = FakeHip()
    return PrefixIndex("pool", buckets=4, device="cpu", _hip=hip, **kw), hip


def test_member_bits_are_stable_and_retired_bits_are_cleared_before_reuse():
    idx, hip = _index()
    assert idx.set_members(["a", "b", "c"]) == [0, 1, 2]
    assert idx.set_members(["c", "a"]) == [2, 0]  # b vanished: bit 1 retired
    assert idx.live_mask == 0b101
    assert idx.set_members(["c", "a", "d"]) == [2, 0, 3]  # fresh bits first
    assert idx.set_members(["b", "c"]) == [4, 2] and not hip.cleared
    names = [f"m{i}" for i in range(64)]
    bits = idx.set_members(names)  # needs retired bits: cleared first, once
    assert sorted(bits) == list(range(64))
    assert len(hip.cleared) == 1
    want = sum(1 << b for b in (0, 1, 2, 3, 4))
    assert hip.cleared[0] & ((1 << 64) - 1) == want
    assert idx.live_mask == -1  # all 64 bits, as an int64
    with pytest.raises(ValueError):
        idx.set_members(names + ["one-too-many"])
    with pytest.raises(ValueError):
        idx.set_members(["x", "x"])


def test_index_clock_and_ttl():
    from aigw.ops.prefix_ref import NEVER

    t = [100.0]
    idx, _ = _index(ttl_s=30, _clock=lambda: t[0])
    assert idx.now() == 0 and idx.ttl == 30
    t[0] = 142.9
    assert idx.now() == 42
    assert _index(ttl_s=None)[0].ttl == NEVER
    assert idx.keys.dtype == torch.int64 and idx.keys.numel() == 4 * 16
    assert idx.stamps.dtype == torch.int32
    with pytest.raises(ValueError):
        _index(block_tokens=12)
