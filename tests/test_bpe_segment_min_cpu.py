"""CPU: the per-segment-minimum merge schedule of the packed BPE window is
equivalent to the wave-wide-minimum schedule it replaces.

A lane-level emulation of bpe_encode_grouped_body (tok / active / myseg per
lane, greedy leftmost selection, the segmented prefix-min exactly as the
kernel computes it) runs both schedules; both must reproduce
BPERef.encode_batch id for id, and the per-segment schedule may never take
more rounds than the wave-wide one for any group."""

import pytest

import bpe_segment_cases as sc
from aigw.ops.bpe_ref import BPERef, make_merges

CASES = sc.cases()


@pytest.fixture(scope="module", params=[8192, 32768])
def ref(request):
    return BPERef(make_merges(request.param, 1355))


def _check(texts, ref):
    want = ref.encode_batch(texts)
    wave, wave_rounds, segs = sc.encode_grouped(texts, ref.rank_of, False)
    seg, seg_rounds, segs2 = sc.encode_grouped(texts, ref.rank_of, True)
    assert wave == want
    assert seg == want
    assert segs == segs2 and len(wave_rounds) == len(seg_rounds)
    worse = [(g, s, w) for g, (s, w) in enumerate(zip(seg_rounds, wave_rounds))
             if s > w]
    assert not worse, worse[:5]
    return wave_rounds, seg_rounds, segs


@pytest.mark.parametrize("name", sorted(CASES))
def test_schedules_match_reference(ref, name):
    _check(CASES[name], ref)


def test_case_texts_are_what_they_claim(ref):
    """The hand-built inputs do exercise what their names say."""
    rank_of = ref.rank_of
    for name, text in sc.SINGLE_GROUP_TEXTS.items():
        _, rounds, segs = sc.encode_grouped([text], rank_of, True)
        if name == "span_65":
            # seven segments in the first group, the last one chunked
            assert segs[0] == 7 and len(text) > 65
            assert sc.segment_starts(text, [0])[:8] == [0, 5, 10, 15, 20, 25, 30, 65]
        else:
            assert len(text) <= 64 and len(segs) == 1 and segs[0] > 1, name
    # the '#' segments merge nothing, their neighbours do
    ids = ref.encode_batch([sc.NO_MERGE_BETWEEN])[0]
    assert ids.count(ord("#")) == 4
    assert len(ref.encode_batch([b" ##"])[0]) == 3
    assert len(ref.encode_batch([b" the"])[0]) < 4
    # several segments reach the same minimum in one round
    wave, seg, _ = _check([sc.SINGLE_GROUP_TEXTS["equal_minima"]], ref)
    assert seg == wave  # identical segments: nothing to gain, nothing lost
    texts = sc.seeded_200()
    assert len(texts) == 200 and all(1 <= len(t) <= 300 for t in texts)


def test_bench_payload_rounds():
    """The benchmark's 4096-token chat text under the serving merge table:
    same ids under both schedules, and the per-segment schedule saves
    rounds (the reason it exists)."""
    import bench

    ref = BPERef(make_merges(32768, 1355))
    text = b"".join(m["content"].encode() + b"\n"
                    for m in bench.build_payload(4096)["messages"])
    wave, seg, segs = _check([text], ref)
    packed = [g for g, s in enumerate(segs) if s > 1]
    mean_wave = sum(wave[g] for g in packed) / len(packed)
    mean_seg = sum(seg[g] for g in packed) / len(packed)
    print(f"{len(text)} B, {len(segs)} groups, {sum(segs)} segments; rounds "
          f"per packed group: wave-wide {mean_wave:.2f}, per-segment {mean_seg:.2f}")
    assert sum(seg) < sum(wave)
