"""CPU proof that the native cache tail's edge cases (tests/probe_tail_cases.py,
run on the GPU by tests/test_gpu_admission_cache_edges.py) are sensitive: on
kernel_checks.EmulatedProbe, a plain fp32 emulation of the tail, every case
passes; with each of twelve deliberately wrong variants of plausible bugs the
case named for it fails, with a message that names the broken property. The
last tests delete one feature of a case at a time and show that the mutant
it was there for then slips through."""

import pytest
import torch

import kernel_checks as kc
import probe_tail_cases as pc

FORMATS = pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])


@pytest.fixture(scope="module")
def data():
    return pc.Data()


def _all_cases(data, rig, fp8):
    yield pc.case_cross_text(data, rig, fp8)
    for column in pc.ONE_ROW_COLUMNS:
        yield pc.case_one_row(data, rig, fp8, column)
    yield pc.case_partial_index(data, rig, fp8)
    for threshold in (-2.0, 0.5):
        yield pc.case_count_edges(data, rig, fp8, threshold=threshold)
    for t in pc.split_thresholds(data, fp8):
        yield pc.case_threshold(data, rig, fp8, t)
    yield pc.case_second_cta(data, rig, fp8)
    yield pc.case_ring_wrap(data, rig, fp8)
    yield pc.case_slots(data, rig, fp8)
    for cache in (True, False):
        yield pc.case_two_sets(data, rig, fp8, cache=cache)


@FORMATS
def test_correct_emulation_passes_every_case(data, fp8):
    worst = max(s.worst for s in _all_cases(data, pc.cpu_rig(data), fp8))
    # the emulation is the plain fp32 yardstick the allowance was measured with
    assert worst <= kc.PROBE_EDGE_MEASURED_FP32_DISAGREEMENT[fp8]


def test_measured_allowances(data):
    """The recorded constants are what the CPU measures: every cell of the
    score matrix of originals, variants and the foreign text; the count-edge
    texts (sequential fp32 mean) measure no worse."""
    e = data.edges()
    short = data.texts + data.variants + [data.foreign]
    for fp8 in (False, True):
        recorded = kc.PROBE_EDGE_MEASURED_FP32_DISAGREEMENT[fp8]
        for texts in (short, e["texts"] + e["variants"]):
            q64 = data.vec(texts, fp8)
            q32 = kc.probe_plain_fp32_sequential(
                [data.ids(t) for t in texts], data.emb, data.proj, fp8).double()
            measured = float((q32 @ q32.T - q64 @ q64.T).abs().max())
            print(f"fp8={fp8} {len(texts)} texts: {measured:.3e} (recorded {recorded:.3e})")
            assert measured <= recorded
            if texts is short:
                assert measured >= 0.95 * recorded
    assert data.counts(e["texts"]) == list(kc.PROBE_EDGE_COUNTS)


# mutant -> (the GPU test whose case catches it, that case, the property its
# rejection names)
CATCHES = {
    "drop_last_token": ("test_cross_text_scores", pc.case_cross_text, "score off"),
    "chunk_first_128": ("test_token_count_edges", pc.case_count_edges, "score off"),
    "mean_div_c_plus_1": ("test_cross_text_scores", pc.case_cross_text, "score off"),
    "pool_prev_request": ("test_cross_text_scores", pc.case_cross_text,
                          "score off|wrong row"),
    "negative_wrong_branch": ("test_one_row_columns[foreign]",
                              lambda d, r, f: pc.case_one_row(d, r, f, "foreign"),
                              "score off|lost hit"),
    "threshold_gt_zero": ("test_threshold_cut",
                          lambda d, r, f: pc.case_threshold(d, r, f, 0.92),
                          "under threshold"),
    "rows_past_1024_unscanned": ("test_second_cta_and_duplicates",
                                 pc.case_second_cta, "wrong row"),
    "ring_wrap_head_plus_1": ("test_ring_wrap", pc.case_ring_wrap, "wrong row"),
    "visible_reset_on_wrap": ("test_ring_wrap", pc.case_ring_wrap, "wrong row"),
    "neg_slot_to_slot0": ("test_pending_slots", pc.case_slots,
                          "wrong row|score off"),
    "identity_slots": ("test_pending_slots", pc.case_slots, "wrong row|score off"),
    "set1_returns_set0": ("test_two_sets", pc.case_two_sets, "counts|wrong row"),
}


def test_every_mutant_has_a_case():
    assert sorted(CATCHES) == sorted(kc.PROBE_TAIL_MUTANTS)


@FORMATS
@pytest.mark.parametrize("mutant", kc.PROBE_TAIL_MUTANTS)
def test_mutants_are_rejected(data, mutant, fp8):
    _, case, names = CATCHES[mutant]
    with pytest.raises(AssertionError, match=names) as exc:
        case(data, pc.cpu_rig(data, mutant), fp8)
    assert "unfit" not in str(exc.value)


def test_threshold_mutant_also_fails_on_negative_scores(data):
    with pytest.raises(AssertionError, match="lost hit"):
        pc.case_one_row(data, pc.cpu_rig(data, "threshold_gt_zero"), False, "foreign")


def test_comparator_refuses_unfit_inputs(data):
    """A lead or a threshold distance under 10x the allowance is refused,
    whatever the probe returned."""
    q = data.vec(data.variants[:4], False)
    inserted = data.vec(data.texts[:4], False)
    ref = kc.probe_ring_reference(inserted, 8, q, -2.0)
    kc.check_probe_lookup(ref["rows"], ref["scores"], ref, 1e-4)
    with pytest.raises(AssertionError, match="unfit.*runner-up"):
        kc.check_probe_lookup(ref["rows"], ref["scores"], ref, 0.05)
    near = kc.probe_ring_reference(inserted, 8, q, ref["scores"][0] - 5e-4)
    with pytest.raises(AssertionError, match="unfit.*threshold"):
        kc.check_probe_lookup(near["rows"], near["scores"], near, 1e-4)
    # a miss is exactly -1 / 0.0, and a right row needs the right score
    high = kc.probe_ring_reference(inserted, 8, q, 1.5)
    assert high["rows"] == [-1] * 4
    with pytest.raises(AssertionError, match="under threshold"):
        kc.check_probe_lookup([-1, -1, -1, 0], [0.0] * 4, high, 1e-4)
    with pytest.raises(AssertionError, match="under threshold"):
        kc.check_probe_lookup([-1] * 4, [0.0, 0.0, 1e-9, 0.0], high, 1e-4)
    off = list(ref["scores"])
    off[2] += 3e-4
    with pytest.raises(AssertionError, match="score off"):
        kc.check_probe_lookup(ref["rows"], off, ref, 1e-4)


def test_ring_reference_model():
    """Wrap, visible clamp, exact duplicates and the threshold, by hand."""
    v = torch.eye(6, dtype=torch.float64)[[0, 1, 2, 1, 3]]  # insert order
    ref = kc.probe_ring_reference(v, 3, torch.eye(6, dtype=torch.float64)[:5], 0.5)
    assert ref["insert_rows"] == [0, 1, 2, 0, 1] and ref["visible"] == 3
    # ring now holds e1, e3, e2 in rows 0, 1, 2; e0 was overwritten
    assert ref["rows"] == [-1, 0, 2, 1, -1]
    assert ref["scores"] == [0.0, 1.0, 1.0, 1.0, 0.0]
    dup = kc.probe_ring_reference(v[[1, 2, 1]], 8, v[[1]], -2.0)
    assert dup["ties"] == [{0, 2}] and dup["gaps"] == [1.0] and dup["visible"] == 3


# --- the case does the work: delete one feature, one mutant slips through ---

@FORMATS
def test_without_long_texts_the_chunk_mutant_passes(data, fp8):
    pc.case_count_edges(data, pc.cpu_rig(data, "chunk_first_128"), fp8, long=False)


@FORMATS
@pytest.mark.parametrize("mutant", ["ring_wrap_head_plus_1", "visible_reset_on_wrap"])
def test_without_a_wrapped_ring_the_ring_mutants_pass(data, mutant, fp8):
    pc.case_ring_wrap(data, pc.cpu_rig(data, mutant), fp8, capacity=400)


@FORMATS
def test_report_what_self_match_lookups_let_through(data, fp8, capsys):
    """The check the suite had before (every text finds its own row, score
    within PROBE_SCORE_ALLOWANCE of the reference self-match), on the old
    130 texts, against the pooling mutants. Printed, not asserted."""
    ids = [data.ids(t) for t in data.texts]
    want = (data.vec(data.texts, fp8) ** 2).sum(dim=1)
    for mutant in kc.PROBE_TAIL_MUTANTS[:4]:
        q = kc.probe_plain_fp32_sequential(ids, data.emb, data.proj, fp8, mutant)
        _, rows, scores = kc.emulate_probe_tail(ids, data.emb, data.proj, fp8, q,
                                                len(ids), -2.0, mutant, q=q)
        wrong = sum(r != i for i, r in enumerate(rows))
        off = sum(abs(s - float(w)) > kc.PROBE_SCORE_ALLOWANCE
                  for s, w in zip(scores, want))
        with capsys.disabled():
            print(f"\nself-match check, {'fp8' if fp8 else 'bf16'}, {mutant}: "
                  f"{wrong} wrong rows, {off} scores off -> "
                  f"{'caught' if wrong or off else 'LET THROUGH'}")
