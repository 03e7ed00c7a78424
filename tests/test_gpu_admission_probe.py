"""GPU: the native admission path (csrc/admission.hip), driven directly
through aigw_fast.AdmissionProbe instead of the HTTP server: per-request
token counts against the CPU BPE oracle at batch sizes that make both
device scans carry across 256-entry chunks, and the native cache's rows
and score VALUES against an fp64 CPU reference that mirrors every rounding
stage of the embed pipeline."""

import numpy as np
import pytest
import torch

import kernel_checks as kc

pytestmark = pytest.mark.gpu

MAX_BYTES = 1 << 17
MAX_REQ = 512


@pytest.fixture(scope="module")
def oracle():
    from aigw.ops.bpe_ref import BPERef, build_hash_table, make_merges

    merges = make_merges(kc.PROBE_N_MERGES, kc.PROBE_SEED)
    keys, ranks = build_hash_table(merges)
    ref = BPERef(merges)
    texts = kc.probe_lookup_texts()
    big = kc.probe_big_batch(texts)
    return {
        "keys": keys, "ranks": ranks, "ref": ref, "texts": texts, "big": big,
        "ids": ref.encode_batch(texts),
        "big_counts": [len(i) for i in ref.encode_batch(big)],
        "weights": kc.probe_weights(256 + kc.PROBE_N_MERGES),
    }


def _probe(oracle):
    import aigw_fast

    return aigw_fast.AdmissionProbe(oracle["keys"], oracle["ranks"],
                                    MAX_BYTES, MAX_REQ, device=0)


def test_probe_counts_match_oracle(oracle):
    """300 texts, > 66 000 bytes (1-byte texts included): more than 256
    entries in the 256-byte-block scans; every count equals the oracle's.
    Smaller batches on the same probe then reuse the (stale) buffers."""
    probe = _probe(oracle)
    big = oracle["big"]
    assert sum(len(t) for t in big) > 256 * 256 and len(big) > 256
    assert probe.count(big) == oracle["big_counts"]
    ref = oracle["ref"]
    for texts in ([b"x"], [b"a", b"b c", b"d"], big[:40], oracle["texts"]):
        assert probe.count(texts) == [len(i) for i in ref.encode_batch(texts)]


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_probe_lookup_rows_and_scores(oracle, fp8):
    """130 distinct texts (two 128-query passes): after inserting every
    text's parked vector, each text must return its own row, with the score
    the fp64 mirrored reference gives (mean -> bf16 -> projection ->
    normalise -> bf16 -> e4m3 for fp8 -> dot) within the CPU-measured
    allowance for rounding-boundary flips. The same texts are then looked
    up from the back of a 300-request batch, behind the per-request scan's
    chunk carry."""
    texts, ids = oracle["texts"], oracle["ids"]
    emb, proj = oracle["weights"]
    allowance = kc.PROBE_SCORE_ALLOWANCE
    st = kc.probe_score_stats(ids, emb, proj, fp8)
    assert st["min_lead"] >= 10 * allowance  # before touching the GPU
    want_counts = [len(i) for i in ids]
    want_scores = st["self"].tolist()

    probe = _probe(oracle)
    probe.init_cache(emb.view(torch.uint16).numpy(), proj.view(torch.uint16).numpy(),
                     capacity=1024, threshold=-2.0, pending_cap=MAX_REQ, fp8=fp8)
    counts, rows, scores = probe.count_lookup(texts)
    assert counts == want_counts
    assert rows == [-1] * len(texts)  # empty index: nothing to return
    assert [probe.insert(i) for i in range(len(texts))] == list(range(len(texts)))
    torch.cuda.synchronize()  # inserts ran on the cache's own stream

    def check(rows, scores, base, what):
        errs = [abs(s - w) for s, w in zip(scores[base:], want_scores)]
        print(f"{what}: max |score - ref| = {max(errs):.3e} "
              f"(allowance {allowance:.3e})")
        assert rows[base:] == list(range(len(texts))), what
        bad = [(i, scores[base + i], want_scores[i]) for i, e in enumerate(errs)
               if e > allowance]
        assert not bad, (what, bad[:5])

    counts, rows, scores = probe.count_lookup(texts)
    assert counts == want_counts
    check(rows, scores, 0, "130-text batch")

    big = oracle["big"]
    counts, rows, scores = probe.count_lookup(big)
    assert counts == oracle["big_counts"]
    check(rows, scores, len(big) - len(texts), "behind 170 fillers")
    assert all(0 <= r < len(texts) for r in rows)
    assert np.isfinite(scores).all()
