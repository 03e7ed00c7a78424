"""GPU: the native semantic-cache tail of csrc/admission.hip at its edges,
through aigw_fast.AdmissionProbe: scores between DIFFERENT texts, one-row
columns with negative scores, a partly filled index, token counts around the
meanpool's block count and staging size, the production threshold cut, a
second top-k CTA with duplicated rows, the ring's wrap, arbitrary and absent
pending slots, and both batch sets in flight at once. Rows are held to the
fp64 argmax of the mirrored reference and scores to it within the
CPU-measured allowance (kernel_checks.PROBE_EDGE_ALLOWANCE); the cases
themselves are in tests/probe_tail_cases.py and are proven to bite on the CPU
by tests/test_kernel_checks_probe_cpu.py."""

import pytest

import probe_tail_cases as pc

pytestmark = pytest.mark.gpu

FORMATS = pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])


@pytest.fixture(scope="module")
def data():
    return pc.Data()


@pytest.fixture(scope="module")
def rig(data):
    return pc.gpu_rig(data)


@FORMATS
def test_cross_text_scores(data, rig, fp8):
    pc.case_cross_text(data, rig, fp8)


@FORMATS
@pytest.mark.parametrize("column", pc.ONE_ROW_COLUMNS)
def test_one_row_columns(data, rig, fp8, column):
    pc.case_one_row(data, rig, fp8, column)


@FORMATS
def test_partial_index(data, rig, fp8):
    pc.case_partial_index(data, rig, fp8)


@FORMATS
@pytest.mark.parametrize("threshold", [-2.0, 0.5])
def test_token_count_edges(data, rig, fp8, threshold):
    pc.case_count_edges(data, rig, fp8, threshold=threshold)


@FORMATS
def test_threshold_cut(data, rig, fp8):
    for t in pc.split_thresholds(data, fp8):  # a median split and 0.92
        pc.case_threshold(data, rig, fp8, t)


@FORMATS
def test_second_cta_and_duplicates(data, rig, fp8):
    pc.case_second_cta(data, rig, fp8)


@FORMATS
def test_ring_wrap(data, rig, fp8):
    pc.case_ring_wrap(data, rig, fp8)


@FORMATS
def test_pending_slots(data, rig, fp8):
    pc.case_slots(data, rig, fp8)


@FORMATS
@pytest.mark.parametrize("cache", [True, False], ids=["cache", "count_only"])
def test_two_sets(data, rig, fp8, cache):
    pc.case_two_sets(data, rig, fp8, cache=cache)
