"""GPU: the admission batcher's lock-free futex waiters (csrc/wake_tree.h)
through the native front. Bursts of 1, 2, 3, 45 and 257 client threads (257 is one
more than the front's batch limit, so one burst spans batches) send texts
of differing lengths; the token counts must equal the CPU BPE reference.

The front reports token counts as totals only, so a burst is checked by its
sum; that every waiter receives its own batch position's values is checked
per waiter by csrc/wake_tree_test.cpp and, here, by the cache case, where a
row or score delivered to the wrong waiter turns a hit into a miss."""

import asyncio
import http.client
import json
import random
import threading
import time

import pytest

pytestmark = pytest.mark.gpu

BURSTS = (1, 2, 3, 45, 257)
# a lost wake-up would surface as collect()'s 30 s deadline
REQUEST_LIMIT_S = 10.0

_JSON_BODY = json.dumps({"id": "x", "object": "chat.completion",
                         "choices": [{"index": 0,
                                      "message": {"role": "assistant",
                                                  "content": "ok"},
                                      "finish_reason": "stop"}]}).encode()
CANNED_JSON = (b"HTTP/1.1 200 OK\r\ncontent-type: application/json\r\n"
               b"content-length: %d\r\n\r\n" % len(_JSON_BODY)) + _JSON_BODY

# SSE without a usage chunk: the gateway's own count is the only source. A
# unary request relayed to this mock gets the same bytes as a buffered body,
# which also carries no usage, so one mock serves mixed bursts.
_FRAMES = (b"data: {\"id\":\"c\",\"object\":\"chat.completion.chunk\","
           b"\"choices\":[{\"index\":0,\"delta\":{\"content\":\"hi\"},"
           b"\"finish_reason\":null}]}\n\n"
           b"data: [DONE]\n\n")
CANNED_SSE = (b"HTTP/1.1 200 OK\r\ncontent-type: text/event-stream\r\n"
              b"transfer-encoding: chunked\r\n\r\n"
              + (b"%x\r\n" % len(_FRAMES)) + _FRAMES + b"\r\n0\r\n\r\n")

_CORPUS = (b"You are a terse assistant. The quick brown fox jumps over the lazy "
           b"dog; numbers 12345 and punctuation!!! mixed,with.commas ") * 12
# 16 texts of differing lengths, 9 .. 1400 bytes
TEXTS = [_CORPUS[i:i + 9 + (i * i * 11) % 1392] for i in range(16)]

_ref_counts = None


def ref_counts():
    """CPU reference count of every text in TEXTS, computed once."""
    global _ref_counts
    if _ref_counts is None:
        from aigw.ops.bpe_ref import BPERef, make_merges

        ref = BPERef(make_merges(8192, 1355))
        # chat text extraction appends one newline per collected value
        _ref_counts = [len(ref.encode_batch([t + b"\n"])[0]) for t in TEXTS]
    return _ref_counts


def burst(port, bodies):
    """One request per thread, all released together. Returns per request
    (status, headers, body, seconds)."""
    n = len(bodies)
    gate = threading.Barrier(n)
    out = [None] * n

    def one(i):
        conn = http.client.HTTPConnection("127.0.0.1", port, timeout=60.0)
        try:
            conn.connect()
            gate.wait()
            t0 = time.monotonic()
            conn.request("POST", "/v1/chat/completions", body=bodies[i],
                         headers={"content-type": "application/json",
                                  "authorization": "Bearer user-a"})
            r = conn.getresponse()
            data = r.read()
            out[i] = (r.status, dict(r.getheaders()), data,
                      time.monotonic() - t0)
        except Exception as e:  # reported by the caller's assertion
            out[i] = (-1, {}, repr(e).encode(), 0.0)
            gate.abort()
        finally:
            conn.close()

    threads = [threading.Thread(target=one, args=(i,)) for i in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for status, _, data, secs in out:
        assert status == 200, data[:200]
        assert secs < REQUEST_LIMIT_S, secs
    return out


def chat_body(text, stream=False):
    payload = {"model": "m",
               "messages": [{"role": "user", "content": text.decode("latin1")}]}
    if stream:
        payload["stream"] = True
    return json.dumps(payload).encode()


def run_front(canned, scenario, **front_kwargs):
    import aigw_fast
    import yaml

    from aigw.extproc.fast_front import FastFront
    from aigw.extproc.server import GatewayServer
    from aigw.filterapi import RuntimeConfig, load_config

    async def run():
        mock = aigw_fast.FastMock()
        up_port = mock.start("127.0.0.1", canned.decode("latin1"))
        cfg = load_config(yaml.safe_load(f"""
routes:
  - name: r
    backends:
      - name: b
        schema: OpenAI
        upstream: {{host: 127.0.0.1, port: {up_port}}}
llmRequestCosts:
  - metadataKey: llm_total_token
    type: TotalToken
"""))
        server = GatewayServer(RuntimeConfig(cfg))
        front = FastFront(server, server.runtime, gpu_direct=True,
                          n_merges=8192, **front_kwargs)
        port = await front.start("127.0.0.1", 0)
        try:
            await asyncio.get_running_loop().run_in_executor(
                None, scenario, front, port)
        finally:
            await front.stop()
            mock.stop()

    asyncio.run(run())


def count_bursts(stream_of):
    """Scenario: every burst size; request i of a burst streams when
    stream_of(i). After each burst the totals must have grown by the
    reference counts of exactly the texts sent."""
    counts = ref_counts()

    def scenario(front, port):
        seen = 0
        for n in BURSTS:
            # rotate so that successive bursts start at different texts
            idx = [(i + n) % len(TEXTS) for i in range(n)]
            burst(port, [chat_body(TEXTS[t], stream=stream_of(i))
                         for i, t in enumerate(idx)])
            seen += sum(counts[t] for t in idx)
            st = front.stats()
            assert st["gpu_tokens"] == seen, (n, st["gpu_tokens"], seen)
            assert st["input_tokens"] == seen, (n, st["input_tokens"], seen)

    return scenario


@pytest.mark.timeout(120)
def test_unary_bursts_sleeping_waiters():
    """Unary requests sleep in collect() until their batch is published."""
    run_front(CANNED_JSON, count_bursts(lambda i: False))


@pytest.mark.timeout(120)
def test_stream_bursts_late_collect():
    """Streamed requests collect after the upstream round trip, so the
    batcher finds no sleeper and makes no wake call."""
    run_front(CANNED_SSE, count_bursts(lambda i: True))


@pytest.mark.timeout(120)
def test_mixed_bursts_sleeping_and_late_waiters_in_one_batch():
    """Unary and streamed requests in one burst: a batch holds sleeping
    waiters next to ones that have not arrived at collect()."""
    run_front(CANNED_SSE, count_bursts(lambda i: i % 3 != 1))


@pytest.mark.timeout(120)
def test_cache_burst_row_score_slot_travel_with_the_count():
    """Native cache on: 45 distinct texts miss and are inserted; a second
    burst repeats 23 of them among 22 new ones. Every repeat must hit and
    every new text must miss, which holds only if each waiter gets its own
    row and score; the counts are checked as in the other cases."""
    from aigw.ops.bpe_ref import BPERef, make_merges

    rng = random.Random(2024)
    alphabet = "abcdefghijklmnopqrstuvwxyz0123456789"

    def distinct_text():
        # few distinct tokens per text, so two texts' pooled embeddings are
        # far below the 0.95 threshold
        word = "".join(rng.choice(alphabet) for _ in range(6))
        return (" ".join([word] * rng.randint(4, 40))).encode()

    first = [distinct_text() for _ in range(45)]
    fresh = [distinct_text() for _ in range(22)]
    assert len({t.split()[0] for t in first + fresh}) == 67
    second = first[:23] + fresh
    order = list(range(45))
    rng.shuffle(order)  # hits and misses interleaved over batch positions
    second = [second[i] for i in order]
    ref = BPERef(make_merges(8192, 1355))
    want = sum(len(ref.encode_batch([t + b"\n"])[0]) for t in first + second)

    def scenario(front, port):
        out = burst(port, [chat_body(t) for t in first])
        assert not any(h.get("x-aigw-cache") == "hit" for _, h, _, _ in out)
        out = burst(port, [chat_body(t) for t in second])
        for t, (_, h, _, _) in zip(second, out):
            assert (h.get("x-aigw-cache") == "hit") == (t in first[:23]), t
        st = front.stats()
        assert st["gpu_tokens"] == want, (st["gpu_tokens"], want)
        assert st["cache_hits"] == 23 and st["cache_misses"] == 67, st

    run_front(CANNED_JSON, scenario, gpu_cache=True, cache_threshold=0.95)
