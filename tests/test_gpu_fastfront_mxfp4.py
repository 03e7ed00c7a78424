"""The native front with an MXFP4 cache index: the command line hands the
dtype down, and a repeat request is served from the in-process cache
(csrc/admission.hip), end to end."""

import argparse
import asyncio
import json

import pytest


def test_cli_hands_mxfp4_to_the_native_front():
    from aigw.cli.main import _check_cache_flags, _fast_front_options

    args = argparse.Namespace(
        front="fast", gpu=True, semantic_cache=True, cache_scope="value", cache_ttl_s=0.0,
        cache_index_dtype="mxfp4", cache_candidates=1, cache_dim=384, workers=1)
    _check_cache_flags(args)
    assert _fast_front_options(args, True) == dict(
        gpu_direct=True, gpu_cache=True, cache_index_dtype="mxfp4")


@pytest.mark.gpu
def test_fast_front_native_cache_mxfp4():
    import aigw_fast
    import torch

    from aigw.extproc.fast_front import FastFront
    from aigw.extproc.server import GatewayServer
    from aigw.extproc.upstream_client import LeanClient
    from aigw.filterapi import RuntimeConfig, load_config
    from aigw.testing.fastmock import canned_chat_response

    payload = json.dumps({"model": "m", "messages": [{
        "role": "user", "content": "what is the airspeed velocity of an unladen swallow " * 20}]})

    async def run():
        mock = aigw_fast.FastMock()
        up_port = mock.start("127.0.0.1", canned_chat_response().decode("latin1"))
        server = GatewayServer(RuntimeConfig(load_config({"routes": [{"name": "r", "backends": [
            {"name": "b", "schema": "OpenAI",
             "upstream": {"host": "127.0.0.1", "port": up_port}}]}]})))
        front = FastFront(server, server.runtime, gpu_direct=True, gpu_cache=True,
                          n_merges=8192, cache_threshold=0.95, cache_index_dtype="mxfp4")
        port = await front.start("127.0.0.1", 0)
        client = LeanClient()
        try:
            for hits in (0, 1):  # cold, then from the native cache
                r = await client.post(host="127.0.0.1", port=port, tls=False,
                                      path="/v1/chat/completions", body=payload.encode(),
                                      headers={"content-type": "application/json"},
                                      timeout_s=60.0)
                data = await r.read()
                r.release()
                assert r.status == 200 and b'"content":"ok"' in data, data[:200]
                assert (r.headers.get("x-aigw-cache") == "hit") == bool(hits), front.stats()
                assert front.stats()["cache_hits"] == hits
                # the insert was launched, on the cache's own stream, before the
                # response left: wait for it, or the repeat may race the row
                torch.cuda.synchronize()
            assert mock.requests() == 1  # (the mock counts after it has answered)
        finally:
            await client.close()
            await front.stop()
            mock.stop()

    asyncio.run(run())
