"""Request text reaches the real in-process admission unchanged: a
FastServer with HIP admission serves three connections of distinct texts
(lengths cycling 1, 15, 16, 17 and 4096 bytes, one in eight with escapes)
and its gpu_tokens total must equal the sum of AdmissionProbe.count() over
the texts the scanner should have extracted. Any torn, stale or misplaced
text in the handoff (connection buffer -> waiter -> staging) changes the
sum."""

import http.client
import json
import threading

import pytest

pytestmark = pytest.mark.gpu

LENS = [1, 15, 16, 17, 4096]
CONNS = 3
PER_CONN = 40
WORDS = ["alpha", "beta", "gamma", "delta", "the", "quick", "brown", "fox"]


def _text(conn, seq):
    """Extracted text for (conn, seq): exactly LENS[...] bytes, ending in the
    newline the scanner appends after a message's content."""
    n = LENS[(conn + seq) % len(LENS)]
    tag = "c%d-s%d: " % (conn, seq)
    fill = " ".join(WORDS[(conn + seq + i) % len(WORDS)] for i in range(n // 3 + 2))
    body = (tag + fill) if n - 1 > len(tag) else fill
    body = body[: n - 1]
    if (conn + seq) % 8 == 0 and n >= 15:
        # characters the JSON body has to escape ('é' is two bytes)
        body = body[:5] + '"\\\n\té' + body[11:]
    assert len(body.encode()) == n - 1
    return body + "\n"


def test_gpu_tokens_match_probe_counts():
    import aigw_fast
    from aigw.ops.bpe_ref import build_hash_table, make_merges

    keys, ranks = build_hash_table(make_merges(8192, 1355))
    resp = json.dumps({"id": "s", "object": "chat.completion", "choices": [],
                       "usage": {"total_tokens": 6}}).encode()
    canned = (b"HTTP/1.1 200 OK\r\ncontent-type: application/json\r\n"
              b"content-length: %d\r\n\r\n" % len(resp)) + resp
    mock = aigw_fast.FastMock()
    up_port = mock.start("127.0.0.1", canned.decode("latin1"))
    srv = aigw_fast.FastServer()
    srv.add_route("handoff", "", 1, True, True,
                  [{"name": "b", "host": "127.0.0.1", "port": up_port}])
    srv.enable_gpu_direct(keys, ranks, device=0)
    port = srv.start("127.0.0.1", 0)

    texts = [[_text(c, s) for s in range(PER_CONN)] for c in range(CONNS)]
    errors = []

    def client(c):
        try:
            h = http.client.HTTPConnection("127.0.0.1", port, timeout=30)
            for t in texts[c]:
                body = json.dumps({"model": "m", "messages": [
                    {"role": "user", "content": t[:-1]}]})
                h.request("POST", "/v1/chat/completions", body=body,
                          headers={"content-type": "application/json"})
                r = h.getresponse()
                r.read()
                if r.status != 200:
                    errors.append((c, r.status))
            h.close()
        except Exception as e:  # surfaced by the assert below
            errors.append((c, repr(e)))

    threads = [threading.Thread(target=client, args=(c,)) for c in range(CONNS)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    try:
        assert not errors, errors[:5]
        got = srv.stats()["gpu_tokens"]
        stats = srv.gpu_direct_stats()
        take_us = srv.gpu_direct_take_us()
    finally:
        srv.stop()
        mock.stop()

    probe = aigw_fast.AdmissionProbe(keys, ranks, 1 << 20, 512, device=0)
    flat = [t for per in texts for t in per]
    want = sum(probe.count(flat))
    print("gpu_tokens=%d probe_sum=%d batches=%d take_us=%d"
          % (got, want, stats[0], take_us))
    assert stats[1] == len(flat) and stats[4] == 0, stats
    assert got == want
