"""GPU: the four-kernel admission submit (csrc/admission_front_kernels.cuh)
through aigw_fast.AdmissionProbe: group heads derived in byte space with a
look-back into the previous 256-byte block, one scan launch and one
compaction pass for segments and groups, 16-byte loads with a byte-wise
tail, a staging buffer restaged between batches and both batch sets in
flight. Counts are checked against the CPU oracle; the cache tail runs
behind the new front end."""

import numpy as np
import pytest
import torch

import kernel_checks as kc

pytestmark = pytest.mark.gpu

MAX_BYTES = 1 << 17
MAX_REQ = 512

# every pair of these letters is a merge of the synthetic table (its 16 x 16
# seed pairs), so a text of two or more of them always has fewer tokens than
# bytes; '#' is in no merge, so a run of it has as many tokens as bytes
_MERGING = b"etaoinshrdlucmfw"
_WORDS = (b"the", b"of", b"a", b"I", b"seventeen", b"42", b"e.g.", b"into",
          b"station", b"\n", b"--", b"x1")


@pytest.fixture(scope="module")
def oracle():
    from aigw.ops.bpe_ref import BPERef, build_hash_table, make_merges

    merges = make_merges(kc.PROBE_N_MERGES, kc.PROBE_SEED)
    keys, ranks = build_hash_table(merges)
    ref = BPERef(merges)
    memo = {}

    def want(texts):
        key = tuple(texts)
        if key not in memo:
            memo[key] = [len(i) for i in ref.encode_batch(list(texts))]
        return memo[key]

    return {"keys": keys, "ranks": ranks, "want": want}


def _probe(oracle):
    import aigw_fast

    return aigw_fast.AdmissionProbe(oracle["keys"], oracle["ranks"],
                                    MAX_BYTES, MAX_REQ, device=0)


@pytest.fixture(scope="module")
def probe(oracle):
    return _probe(oracle)


@pytest.fixture(scope="module")
def big(oracle):
    texts = kc.probe_big_batch(kc.probe_lookup_texts())
    assert len(texts) == 300 and sum(len(t) for t in texts) > 66000
    return texts


def _check(probe, oracle, texts):
    want = oracle["want"](texts)
    assert probe.count(texts) == want
    return want


def _merging(n: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    return bytes(_MERGING[int(i)] for i in rng.integers(0, len(_MERGING), n))


def _prose(n: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    words = [_WORDS[int(i)] for i in rng.integers(0, len(_WORDS), n // 2 + 1)]
    return b" ".join(words)[:n]


def _one_letter_words(n: int, seed: int) -> bytes:
    """'e t a o ...': a segment start at every other byte, 16 per cell."""
    return b" ".join(bytes([b]) for b in _merging(n // 2 + 1, seed))[:n]


def _xy():
    """Two batches of equal text lengths whose every count differs."""
    lengths = [2, 3, 17, 40, 255, 256, 257, 700, 31, 5]
    x = [_merging(n, 300 + i) for i, n in enumerate(lengths)]
    y = [b"#" * n for n in lengths]
    return x, y


def test_restaging_follows_the_bytes_just_staged(probe, oracle):
    x, y = _xy()
    want_x, want_y = oracle["want"](x), oracle["want"](y)
    assert [len(t) for t in x] == [len(t) for t in y]
    assert all(a != b for a, b in zip(want_x, want_y))
    for batch, want in ((x, want_x), (y, want_y), (x, want_x)):
        assert probe.count(batch) == want  # set 0
    for batch, want in ((x, want_x), (y, want_y), (x, want_x)):
        probe.submit(1, batch)
        assert probe.wait(1)[0] == want


@pytest.mark.parametrize("first", [0, 1])
def test_interleaved_sets(probe, oracle, first):
    x, y = _xy()
    want = [oracle["want"](x), oracle["want"](y)]
    probe.submit(0, x)
    probe.submit(1, y)
    for s in (first, 1 - first):
        assert probe.wait(s)[0] == want[s]


SIZES = [1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4097]


def _cuts(n: int):
    cuts = []
    for c in (max(1, n // 3), max(1, 2 * n // 3)):
        if c % 16 == 0:
            c += 1
        cuts.append(c)
    assert all(c % 16 != 0 and c <= n for c in cuts) and cuts[0] <= cuts[1]
    return cuts


@pytest.mark.parametrize("n", SIZES)
def test_total_sizes(probe, oracle, n):
    text = _prose(n, 40 + n)
    assert len(text) == n
    _check(probe, oracle, [text])
    a, b = _cuts(n)
    _check(probe, oracle, [text[:a], text[a:b], text[b:]])


@pytest.mark.parametrize("empty_before", [False, True], ids=["plain", "empty"])
@pytest.mark.parametrize("off", [250, 251, 255, 256, 257])
def test_cell_straddles_block_boundary(probe, oracle, off, empty_before):
    """The second request starts at `off`; its cells are relative to `off`,
    so one of them straddles byte 256 (or, at 256, starts on it) and its
    group head is decided from segment starts of the block before."""
    texts = [_one_letter_words(off, 11)]
    if empty_before:
        texts.append(b"")
    texts.append(_one_letter_words(300, 12))
    _check(probe, oracle, texts)


def test_handback_512_requests_3_non_empty(probe, oracle):
    texts = [b""] * 512
    texts[0], texts[255], texts[511] = b"hello there", b"x", _prose(300, 5)
    want = _check(probe, oracle, texts)
    assert sum(1 for w in want if w) == 3


def test_handback_300_short_requests(probe, oracle):
    texts = [_prose(1 + i % 7, 900 + i) for i in range(300)]
    want = _check(probe, oracle, texts)
    assert all(w > 0 for w in want)


def test_handback_one_bpe_block_and_many(probe, oracle, big):
    small = [b"twenty bytes of text", b"and twenty more here"]
    assert sum(map(len, small)) // 32 + len(small) + 1 <= 8  # one block
    _check(probe, oracle, small)
    _check(probe, oracle, big)  # > 2000 groups: hundreds of blocks


def test_stale_state(oracle, big):
    """Big batch, a tiny one, the big one again on ONE fresh probe: flags,
    block counts or request counts left over from the batch before would
    show in the counts."""
    probe = _probe(oracle)
    _check(probe, oracle, big)
    _check(probe, oracle, [b"a", b"b c", b"d"])
    _check(probe, oracle, big)


@pytest.mark.parametrize("fmt", [{"fp8": False}, {"fp8": False, "mxfp4": True}],
                         ids=["bf16", "mxfp4"])
def test_cache_tail_behind_the_front_end(oracle, fmt):
    texts = kc.probe_lookup_texts()
    want = oracle["want"](texts)
    emb, proj = kc.probe_weights(256 + kc.PROBE_N_MERGES)
    probe = _probe(oracle)
    probe.init_cache(emb.view(torch.uint16).numpy(), proj.view(torch.uint16).numpy(),
                     capacity=1024, threshold=-2.0, pending_cap=MAX_REQ, **fmt)
    counts, rows, _ = probe.count_lookup(texts)
    assert counts == want and rows == [-1] * len(texts)
    assert [probe.insert(i) for i in range(len(texts))] == list(range(len(texts)))
    torch.cuda.synchronize()  # inserts ran on the cache's own stream
    counts, rows, _ = probe.count_lookup(texts)
    assert counts == want
    assert rows == list(range(len(texts)))
