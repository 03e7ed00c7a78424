"""GPU: the fused front end of the native admission pipeline
(seg_flags_count_kernel, group_flags_count_kernel in csrc/bpe_kernels.cuh),
driven through aigw_fast.AdmissionProbe: forced request starts at and
around a 256-byte block boundary, empty requests sharing one offset, more
requests than bytes, buffers left stale by an earlier batch, and the cache
tail behind the new front end. Counts are checked against the CPU oracle."""

import pytest
import torch

import bpe_segment_cases as sc
import kernel_checks as kc

pytestmark = pytest.mark.gpu

MAX_BYTES = 1 << 17
MAX_REQ = 512


@pytest.fixture(scope="module")
def oracle():
    from aigw.ops.bpe_ref import BPERef, build_hash_table, make_merges

    merges = make_merges(kc.PROBE_N_MERGES, kc.PROBE_SEED)
    keys, ranks = build_hash_table(merges)
    return {"keys": keys, "ranks": ranks, "ref": BPERef(merges)}


def _probe(oracle):
    import aigw_fast

    return aigw_fast.AdmissionProbe(oracle["keys"], oracle["ranks"],
                                    MAX_BYTES, MAX_REQ, device=0)


@pytest.fixture(scope="module")
def probe(oracle):
    return _probe(oracle)


def _check(probe, oracle, texts):
    want = [len(i) for i in oracle["ref"].encode_batch(texts)]
    assert probe.count(texts) == want
    return want


# letters only: no class change and no space, so the text boundary has no
# natural segment start and only the forced start splits the texts
FORCED = {
    "boundary_255": [255, 40, 30],
    "boundary_256": [256, 40, 30],
    "boundary_257": [257, 40, 30],
    "boundaries_255_256_257": [255, 1, 1, 50],
}


@pytest.mark.parametrize("name", sorted(FORCED))
def test_forced_starts_around_block_boundary(probe, oracle, name):
    texts = [sc.letters(n, 100 + i) for i, n in enumerate(FORCED[name])]
    from aigw.ops.bpe_ref import segment_starts

    offs = [sum(FORCED[name][:i]) for i in range(len(texts))]
    assert segment_starts(b"".join(texts), [0]) == [0]
    assert segment_starts(b"".join(texts), offs) == offs
    _check(probe, oracle, texts)


@pytest.mark.parametrize("n_empty", [2, 3])
@pytest.mark.parametrize("prefix", [256, 100], ids=["at_block", "off_block"])
def test_empty_texts_sharing_an_offset(probe, oracle, prefix, n_empty):
    texts = ([sc.letters(prefix, 7)] + [b""] * n_empty + [sc.letters(20, 8)])
    want = _check(probe, oracle, texts)
    assert want[1:1 + n_empty] == [0] * n_empty and want[-1] > 0


@pytest.mark.parametrize("where", [0, 150, 299])
def test_more_requests_than_bytes(probe, oracle, where):
    texts = [b""] * 300
    texts[where] = b"hello"
    want = _check(probe, oracle, texts)
    assert sum(1 for w in want if w == 0) == 299


def test_stale_buffers(oracle):
    """Big batch, two small ones, the big one again on ONE probe: a group
    flag or a request count that the fused kernels fail to rewrite would
    carry over from the batch before."""
    probe = _probe(oracle)
    big = kc.probe_big_batch(kc.probe_lookup_texts())
    assert len(big) == 300 and sum(len(t) for t in big) > 66000
    big_want = [len(i) for i in oracle["ref"].encode_batch(big)]
    assert probe.count(big) == big_want
    _check(probe, oracle, [b"a", b"b c", b"d"])
    _check(probe, oracle, big[:40])
    assert probe.count(big) == big_want


def test_cache_tail_behind_fused_front_end(oracle):
    """One lookup round on the texts of test_probe_lookup_rows_and_scores:
    the cache tail still finds every token (counts) and every text its
    own row."""
    texts = kc.probe_lookup_texts()
    want = [len(i) for i in oracle["ref"].encode_batch(texts)]
    emb, proj = kc.probe_weights(256 + kc.PROBE_N_MERGES)
    probe = _probe(oracle)
    probe.init_cache(emb.view(torch.uint16).numpy(), proj.view(torch.uint16).numpy(),
                     capacity=1024, threshold=-2.0, pending_cap=MAX_REQ, fp8=False)
    counts, rows, _ = probe.count_lookup(texts)
    assert counts == want and rows == [-1] * len(texts)
    assert [probe.insert(i) for i in range(len(texts))] == list(range(len(texts)))
    torch.cuda.synchronize()  # inserts ran on the cache's own stream
    counts, rows, _ = probe.count_lookup(texts)
    assert counts == want
    assert rows == list(range(len(texts)))
