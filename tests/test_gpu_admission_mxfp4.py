"""GPU: the native cache with an MXFP4 index (AdmissionProbe, mxfp4=True)
against plain fp64: the parked bf16 vector (kc.probe_reference) quantised by
aigw.ops.mxfp4_ref, scored (dequantised row . e4m3 query) * inv_norm over the
ring model of kc.probe_ring_reference. MEASURED and the leads the row checks
rely on: profiles/admission_mxfp4.md."""

import numpy as np
import pytest
import torch

import kernel_checks as kc
import probe_tail_cases as ptc
from aigw.ops import mxfp4_ref

pytestmark = pytest.mark.gpu

MEASURED = 1.44e-7  # largest |score - reference| over these cases on an MI355X
ALLOWANCE = 4 * MEASURED  # as PROBE_EDGE_ALLOWANCE
R, F = list(range(130)), 130  # the lookup texts by number; the foreign text
# capacity, threshold, batches parked as (texts, slots), slots inserted in
# order, queries, their rows (None: an overwritten text, the reference's row)
CASES = {
    "one row": (1024, -2.0, [(R[:1], R[:1])], R[:1], R[:1], R[:1]),
    "partial 16-row tile": (1024, -2.0, [(R[:17], R[:17])], R[:17], R[:17], R[:17]),
    "two query chunks": (1024, -2.0, [(R, R)], R, R, R),
    # a CTA takes 1024 rows. Eight copies and five more rows: the highest copy
    # wins (the tie rule), at the end of CTA 0, in CTA 1 and in a last tile of 5
    "second CTA, last tile, ties": (2048, -2.0, [(R, R)], R * 8 + R[:5], R,
                                    list(range(1040, 1045)) + list(range(915, 1040))),
    "ring wrap": (64, -2.0, [(R[:70], R[:70])], R[:70], R[:70],
                  [None] * 6 + R[6:64] + R[:6]),
    "foreign text under 0.92": (1024, 0.92, [(R[:17], R[:17])], R[:17], [F] + R[:17],
                                [-1] + R[:17]),
    # -1 parks nothing; slot 9, named again by the later batch, holds text 10
    "pending slots": (1024, -2.0, [(R[:4], [3, -1, 9, 5]), ([10, 11], [9, -1])],
                      [3, 9, 5], [0, 10, 3], [0, 1, 2]),
}


data = pytest.fixture(scope="module")(lambda: ptc.Data())


def new_probe(data, capacity, threshold, proj=None, **fmt):
    probe = ptc.gpu_rig(data).new_probe()
    proj = data.proj if proj is None else proj
    probe.init_cache(data.emb.view(torch.uint16).numpy(), proj.view(torch.uint16).numpy(),
                     capacity=capacity, threshold=threshold, pending_cap=ptc.PENDING, **fmt)
    return probe


@pytest.mark.parametrize("case", CASES)
def test_lookup(data, case):
    cap, threshold, batches, inserts, queries, want_rows = CASES[case]
    text = (data.texts + [data.foreign]).__getitem__
    probe = new_probe(data, cap, threshold, fp8=False, mxfp4=True)
    parked = {}
    for texts, slots in batches:
        _, rows, scores = probe.count_lookup([text(t) for t in texts], slots)
        assert rows == [-1] * len(texts) and scores == [0.0] * len(texts)  # empty index
        parked.update({s: t for t, s in zip(texts, slots) if s >= 0})
    for k, s in enumerate(inserts):
        assert probe.insert(s) == k % cap
    torch.cuda.synchronize()  # inserts ran on the cache's own stream
    packed, scale, inv = mxfp4_ref.quantize(data.vec(data.texts, False).numpy())
    stored = mxfp4_ref.dequantize(packed, scale) * inv.astype(np.float64)[:, None]
    index = torch.from_numpy(stored)[[parked[s] for s in inserts]]
    ref = kc.probe_ring_reference(index, cap, data.vec([text(t) for t in queries], True),
                                  threshold)
    _, rows, scores = probe.count_lookup([text(t) for t in queries], [-1] * len(queries))
    err = max(abs(s - w) for s, w in zip(scores, ref["scores"]))
    print(f"{case}: max |score - ref| = {err:.3e}, min lead {min(ref['gaps']):.3e}")
    # rows are exact where lead and distance from the threshold allow it
    sure = [b for b in range(len(queries))
            if min(ref["gaps"][b], ref["margins"][b]) > 2 * ALLOWANCE]
    assert len(sure) >= 0.95 * len(queries), "too few queries with a safe lead"
    for b in sure:
        own = max(ref["ties"][b]) if ref["rows"][b] >= 0 else -1
        assert want_rows[b] in (None, own), "the ring model"
        assert rows[b] == own, (b, rows[b], scores[b], own, ref["scores"][b])
    assert err <= ALLOWANCE  # under the threshold 0.0 on both sides


def test_refusals(data):
    with pytest.raises(RuntimeError, match="two index formats"):
        new_probe(data, 64, -2.0, fp8=True, mxfp4=True)
    with pytest.raises(RuntimeError, match="shape mismatch"):  # dim 256
        new_probe(data, 64, -2.0, proj=data.proj[:256, :256].contiguous(), mxfp4=True,
                  fp8=False)
