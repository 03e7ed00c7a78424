"""GPU: the per-segment-minimum merge loop of the packed BPE window
(bpe_merge_lanes<true>) against the CPU oracle, through both users of the
kernel header: the torch extension (GPUTokenizer: ids and counts) and the
native admission path (AdmissionProbe: counts). The inputs are single
groups of a few bytes in which several segments merge in the same round
(tests/bpe_segment_cases.py); tests/test_bpe_segment_min_cpu.py checks the
same texts against a lane-level emulation without a GPU."""

import pytest

import bpe_segment_cases as sc

pytestmark = pytest.mark.gpu

CASES = sc.cases()


@pytest.fixture(scope="module", params=[8192, 32768])
def env(request):
    import aigw_fast
    from aigw.ops.bpe_ref import build_hash_table
    from aigw.ops.tokenizer import GPUTokenizer

    tok = GPUTokenizer(n_merges=request.param, device="cuda")
    keys, ranks = build_hash_table(tok.merges)
    probe = aigw_fast.AdmissionProbe(keys, ranks, 1 << 17, 512, device=0)
    ref = tok.reference()
    want = {name: ref.encode_batch(texts) for name, texts in CASES.items()}
    return {"tok": tok, "probe": probe, "want": want}


@pytest.mark.parametrize("name", sorted(CASES))
def test_ids_and_counts_match_reference(env, name):
    texts, want = CASES[name], env["want"][name]
    counts, ids, _ = env["tok"].encode_batch(texts, return_ids=True)
    assert ids == want
    assert counts.cpu().tolist() == [len(w) for w in want]
    assert env["probe"].count(texts) == [len(w) for w in want]
