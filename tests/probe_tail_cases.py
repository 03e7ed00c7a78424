"""The native cache tail's edge cases, written once against the
AdmissionProbe interface (no tests here): tests/test_gpu_admission_cache_edges.py
runs them on aigw_fast.AdmissionProbe, tests/test_kernel_checks_probe_cpu.py
on kernel_checks.EmulatedProbe and its deliberately wrong variants. What a
case expects comes from the CPU oracle and the fp64 mirrored reference
alone (kernel_checks.probe_ring_reference), never from the probe it drives.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import kernel_checks as kc

MAX_BYTES = 1 << 17
MAX_REQ = 512
PENDING = 512


class Data:
    """Texts, oracle ids and fp64 reference vectors, computed once."""

    def __init__(self):
        from aigw.ops.bpe_ref import BPERef, build_hash_table, make_merges

        merges = make_merges(kc.PROBE_N_MERGES, kc.PROBE_SEED)
        self.keys, self.ranks = build_hash_table(merges)
        self.ref = BPERef(merges)
        self.emb, self.proj = kc.probe_weights(256 + kc.PROBE_N_MERGES)
        self.texts = kc.probe_lookup_texts()
        self.variants = kc.probe_variant_texts(self.texts)
        self.fillers = kc.probe_big_batch([])
        # bytes no lookup text holds: near-orthogonal to all of them, so about
        # half of its scores are below zero
        self.foreign = kc._draw(bytes(range(0xF0, 0x100)), 40, 4200)
        self._ids, self._vec = {}, {}
        self.q_cache = {}  # EmulatedProbe's fp32 embeds, by (fp8, text)
        self._edges = {}

    def edges(self, long=True):
        if long not in self._edges:
            self._edges[long] = kc.probe_count_edge_texts(self.ref, long)
        return self._edges[long]

    def ids(self, text):
        if text not in self._ids:
            self._ids[text] = self.ref.encode_batch([text])[0]
        return self._ids[text]

    def counts(self, texts):
        return [len(self.ids(t)) for t in texts]

    def vec(self, texts, fp8):
        """fp64 mirrored reference vectors; a text without tokens pools
        nothing and embeds to the zero vector."""
        missing = [t for t in dict.fromkeys(texts)
                   if (fp8, t) not in self._vec and self.ids(t)]
        if missing:
            v = kc.probe_reference([self.ids(t) for t in missing], self.emb,
                                   self.proj, fp8)
            self._vec.update({(fp8, t): v[i] for i, t in enumerate(missing)})
        zero = torch.zeros(kc.PROBE_DIM, dtype=torch.float64)
        return torch.stack([self._vec[(fp8, t)] if self.ids(t) else zero
                            for t in texts])


class Rig:
    """Where a case gets its probe from, and how it waits for inserts."""

    def __init__(self, new_probe, sync=lambda: None):
        self.new_probe, self.sync = new_probe, sync


def gpu_rig(data):
    import aigw_fast

    def new_probe():
        return aigw_fast.AdmissionProbe(data.keys, data.ranks, MAX_BYTES,
                                        MAX_REQ, device=0)

    return Rig(new_probe, torch.cuda.synchronize)


def cpu_rig(data, mutant=None):
    return Rig(lambda: kc.EmulatedProbe(data.ids, data.emb, data.proj, MAX_REQ,
                                        mutant, data.q_cache))


class Session:
    """One probe with the CPU model of what it was told: the vector parked
    in every pending slot and the vectors inserted so far, in order."""

    def __init__(self, data, rig, fp8, capacity=1024, threshold=-2.0, cache=True):
        self.data, self.rig, self.fp8 = data, rig, fp8
        self.cap, self.threshold = capacity, threshold
        self.allowance = kc.PROBE_EDGE_ALLOWANCE[fp8]
        self.probe = rig.new_probe()
        self.cache = cache
        if cache:
            self.probe.init_cache(
                data.emb.view(torch.uint16).numpy(),
                data.proj.view(torch.uint16).numpy(), capacity=capacity,
                threshold=threshold, pending_cap=PENDING, fp8=fp8)
        self.parked, self.inserted = {}, []
        self.in_flight = {}
        self.worst = 0.0

    def _inserted(self):
        if not self.inserted:
            return torch.zeros(0, kc.PROBE_DIM, dtype=torch.float64)
        return torch.stack(self.inserted)

    def reference(self, texts):
        return kc.probe_ring_reference(self._inserted(), self.cap,
                                       self.data.vec(texts, self.fp8),
                                       self.threshold)

    def fit(self, texts):
        """The texts the comparator would not refuse (reference only)."""
        keep = kc.probe_fit_queries(self.reference(texts), self.allowance)
        return [texts[b] for b in keep]

    def _park(self, texts, slots):
        if slots is None:
            slots = range(len(texts))
        for t, s in zip(texts, slots):
            if s >= 0:
                self.parked[s] = self.data.vec([t], self.fp8)[0]

    def _check(self, got, texts, ref, what, check_from):
        counts, rows, scores = got
        assert counts == self.data.counts(texts), f"counts: {what}"
        if not self.cache:
            assert rows is None and scores is None, f"count-only batch: {what}"
            return None
        part = {k: (v[check_from:] if isinstance(v, list) else v)
                for k, v in ref.items() if k != "insert_rows"}
        try:
            st = kc.check_probe_lookup(rows[check_from:], scores[check_from:],
                                       part, self.allowance)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from None
        self.worst = max(self.worst, st["max_err"])
        print(f"{what}: max |score - ref| = {st['max_err']:.3e} (allowance "
              f"{self.allowance:.3e}), min lead {st['min_gap']:.3e}")
        return ref

    def lookup(self, texts, what, slots=None, check_from=0):
        ref = self.reference(texts)
        got = self.probe.count_lookup(texts) if slots is None else \
            self.probe.count_lookup(texts, slots)
        self._park(texts, slots)
        return self._check(got, texts, ref, what, check_from), got

    def submit(self, s, texts, slots=None):
        ref = self.reference(texts) if self.cache else None
        self.probe.submit(s, texts) if slots is None else \
            self.probe.submit(s, texts, slots)
        if self.cache:
            self._park(texts, slots)
        self.in_flight[s] = (texts, ref)

    def wait(self, s, what, check_from=0):
        texts, ref = self.in_flight.pop(s)
        return self._check(self.probe.wait(s), texts, ref, what, check_from)

    def insert(self, slot):
        want = len(self.inserted) % self.cap
        self.inserted.append(self.parked[slot])
        row = self.probe.insert(slot)
        assert row == want, f"insert row: got {row}, ring model {want}"
        return row

    def insert_all(self, slots):
        rows = [self.insert(s) for s in slots]
        self.rig.sync()  # inserts ran on the cache's own stream
        return rows


def _variant_rows(s, data):
    """The reference itself says each variant's best row is its original."""
    ref = s.reference(data.variants)
    assert ref["rows"] == list(range(len(data.texts)))
    return ref


def case_cross_text(data, rig, fp8):
    """Originals inserted, variants looked up: the original's row and the
    cross score; again behind the 170 fillers (both scans carry)."""
    s = Session(data, rig, fp8)
    ref, got = s.lookup(data.texts, "empty index")
    assert got[1] == [-1] * 130
    assert s.insert_all(range(130)) == list(range(130))
    ref = _variant_rows(s, data)
    assert 0.5 < min(ref["scores"]) and max(ref["scores"]) < 1.01
    s.lookup(data.variants, "130 variants")
    s.lookup(data.fillers + data.variants, "variants behind 170 fillers",
             check_from=170)
    return s


# the only two originals whose column holds scores below zero (the lookup
# texts share digit and space-letter tokens, so nearly every cell is
# positive), and the foreign text, negative against about half the queries
ONE_ROW_COLUMNS = (111, 113, "foreign")


def case_one_row(data, rig, fp8, column):
    """One inserted row: every original and variant returns row 0 with its
    score against that row, the negative ones included."""
    s = Session(data, rig, fp8)
    text = data.foreign if column == "foreign" else data.texts[column]
    s.lookup([text], "park", slots=[7])
    assert s.insert_all([7]) == [0]
    queries = data.texts + data.variants
    ref = s.reference(queries)
    assert ref["rows"] == [0] * 260
    negatives = sum(x < 0 for x in ref["scores"])
    assert negatives >= (60 if column == "foreign" else 1), "column without negative scores"
    s.lookup(queries, f"column {column}", slots=[-1] * 260)
    return s


def case_partial_index(data, rig, fp8):
    """Lookups while the index holds 1, 15, 16 and 17 rows; the reference
    sees the visible rows only."""
    s = Session(data, rig, fp8)
    s.lookup(data.texts, "park")
    queries = data.texts + data.variants
    for n in range(1, 18):
        s.insert_all([n - 1])
        if n in (1, 15, 16, 17):
            fit = s.fit(queries)
            ref = s.reference(fit)
            assert len(fit) >= 100 and n - 1 in ref["rows"]
            s.lookup(fit, f"{n} rows", slots=[-1] * len(fit))
    return s


def case_count_edges(data, rig, fp8, long=True, threshold=-2.0):
    """Token counts 1, 31..33 and 4095..4097, 4227 with an empty request in
    the middle of the batch: oracle counts, rows and cross scores; the
    empty request scores exactly 0.0 (-1 / 0.0 under a threshold of 0.5)."""
    e = data.edges(long)
    n = len(e["texts"])
    batch = e["texts"][:n // 2] + [b""] + e["texts"][n // 2:] + e["variants"]
    assert data.counts(batch)[:n + 1] == (
        e["counts"][:n // 2] + [0] + e["counts"][n // 2:])
    s = Session(data, rig, fp8, threshold=threshold)
    s.lookup(batch, "empty index")
    own = [i for i in range(n + 1) if i != n // 2]
    s.insert_all(own)
    ref = kc.probe_ring_reference(s._inserted(), s.cap, data.vec(batch, fp8), -2.0)
    assert ref["rows"][n + 1:] == list(range(n))  # each variant: its original
    assert [ref["rows"][i] for i in own] == list(range(n))
    assert ref["ties"][n // 2] == set(range(n))  # zero query: every row ties at 0.0
    _, got = s.lookup(batch, f"count edges, threshold {threshold}")
    row, score = got[1][n // 2], got[2][n // 2]
    if threshold <= 0:
        assert 0 <= row < n and score == 0.0, f"empty request: {row} / {score!r}"
    else:
        assert row == -1 and score == 0.0, f"empty request: {row} / {score!r}"
    return s


def split_thresholds(data, fp8):
    """The middle of the widest gap in the central half of the variants'
    sorted reference best scores, and production's 0.92. Variants whose
    best score is within 10x the allowance of the threshold are left out by
    the case (from the reference alone); both sides stay populated."""
    q = data.vec(data.variants, fp8)
    o = data.vec(data.texts, fp8)
    best = np.sort((q @ o.T).max(dim=1).values.numpy())
    lo, hi = len(best) // 4, 3 * len(best) // 4
    k = lo + int(np.argmax(np.diff(best[lo:hi + 1])))
    return [float(best[k] + best[k + 1]) / 2, 0.92]


def case_threshold(data, rig, fp8, threshold):
    """Variants over the threshold return row and score, variants under it
    exactly -1 / 0.0; every original is over it."""
    s = Session(data, rig, fp8, threshold=threshold)
    s.lookup(data.texts, "park")
    s.insert_all(range(130))
    fit = s.fit(data.variants)
    ref = s.reference(fit)
    hits = sum(r >= 0 for r in ref["rows"])
    assert hits >= 5 and len(fit) - hits >= 5, (hits, len(fit))  # both sides
    s.lookup(fit, f"{len(fit)} variants at threshold {threshold:.4f}, {hits} over",
             slots=[-1] * len(fit))
    fit = s.fit(data.texts)
    assert len(fit) >= 100
    s.lookup(fit, "originals", slots=[-1] * len(fit))
    return s


def case_second_cta(data, rig, fp8):
    """Capacity 2048: seven copies of the originals (rows 0..909), then the
    variants (rows 910..1039): rows 1024..1039 belong to the second CTA."""
    s = Session(data, rig, fp8, capacity=2048)
    s.lookup(data.texts, "park originals")
    for _ in range(7):
        for i in range(130):
            s.insert(i)
    s.rig.sync()
    s.lookup(data.variants, "variants before their own rows")
    assert s.insert_all(range(130)) == list(range(910, 1040))
    fit = s.fit(data.variants)
    ref = s.reference(fit)
    assert ref["rows"] == [910 + data.variants.index(t) for t in fit]
    assert len(fit) >= 40 and sum(r >= 1024 for r in ref["rows"]) >= 4
    s.lookup(fit, "variants, own rows 910..1039", slots=[-1] * len(fit))
    fit = s.fit(data.texts)
    ref = s.reference(fit)
    assert len(fit) >= 40 and all(len(t) == 7 for t in ref["ties"])
    s.lookup(fit, "originals, seven copies each", slots=[-1] * len(fit))
    return s


def case_ring_wrap(data, rig, fp8, capacity=200):
    """Capacity 200: originals then variants; the variants wrap over rows
    0..59. One more insert leaves the visible count at the capacity."""
    s = Session(data, rig, fp8, capacity=capacity)
    s.lookup(data.texts, "park originals")
    rows = s.insert_all(range(130))
    s.lookup(data.variants, "variants, originals only")
    rows += s.insert_all(range(130))
    wrapped = capacity < 260
    if wrapped:
        assert capacity == 200 and rows == list(range(200)) + list(range(60))
    for extra in (False, True):
        if extra:
            s.insert_all([0])  # variant 0 once more
        fit = s.fit(data.texts)
        ref = s.reference(fit)
        at = {data.texts.index(t): r for t, r in zip(fit, ref["rows"])}
        if wrapped and not extra:
            # overwritten originals resolve to their variant's row
            assert all(at[i] == 130 + i for i in at if i < 60)
            assert all(at[i] == i for i in at if i >= 60)
            assert sum(i < 60 for i in at) >= 15 and sum(i >= 60 for i in at) >= 25
        s.lookup(fit, f"originals{' after one more insert' if extra else ''}",
                 slots=[-1] * len(fit))
        fit = s.fit(data.variants)
        assert len(fit) >= 40
        s.lookup(fit, "variants, own ring rows", slots=[-1] * len(fit))
    assert s.reference(data.texts[:1])["visible"] == min(capacity, 261)
    return s


def case_slots(data, rig, fp8):
    """A seeded permutation of pending slots with every seventh -1; slots
    that the batch does not name keep an earlier batch's vectors."""
    s = Session(data, rig, fp8)
    s.lookup(data.variants, "earlier batch, identity slots")
    rng = np.random.default_rng(77)
    slots = [int(x) for x in rng.permutation(np.arange(1, PENDING))[:130]]
    slots = [-1 if i % 7 == 0 else x for i, x in enumerate(slots)]
    # (their originals are not inserted: every seventh text parks nothing)
    kept = [x for x in range(7, 130, 7) if x not in slots][:3]
    assert 0 not in slots and len(kept) == 3 and slots.count(-1) == 19
    for bad in ([PENDING] + slots[1:], [-2] + slots[1:],
                slots[:5] + [slots[1]] + slots[6:], slots[:-1]):
        with pytest.raises(Exception):
            s.probe.count_lookup(data.texts, bad)
    s.lookup(data.texts, "permuted slots", slots=slots)
    order = [x for x in slots if x >= 0]
    rng.shuffle(order)
    s.insert_all([int(x) for x in order])
    # slot 0 and three more that this batch did not name: still the variants
    s.insert_all([0] + kept)
    queries = s.fit(data.texts + [data.variants[i] for i in [0] + kept])
    ref = s.reference(queries)
    for i in [0] + kept:
        b = queries.index(data.variants[i])
        assert ref["rows"][b] == len(order) + ([0] + kept).index(i)
    assert len(queries) >= 40
    s.lookup(queries, "each text at its own slot's row", slots=[-1] * len(queries))
    return s


def case_two_sets(data, rig, fp8, cache=True):
    """Set 1 before set 0 was ever used, with the 300-text batch; then one
    batch in flight on each set, collected in the other order."""
    s = Session(data, rig, fp8, cache=cache)
    big = data.fillers + data.texts
    with pytest.raises(Exception):
        s.probe.wait(1)
    s.submit(1, big)
    with pytest.raises(Exception):
        s.probe.submit(1, data.texts)
    s.wait(1, "300 texts on set 1")
    if cache:
        s.insert_all(range(170, 300))
    s.submit(1, big)
    s.wait(1, "300 texts on set 1, index filled", check_from=170)
    a = data.variants
    b = data.fillers[:20] + data.texts[40:110]
    s.submit(0, a, list(range(130)) if cache else None)
    s.submit(1, b, list(range(200, 290)) if cache else None)
    with pytest.raises(Exception):
        s.probe.submit(0, b)
    s.wait(1, "set 1 (90 texts) while set 0 is in flight", check_from=20)
    s.wait(0, "set 0 (130 texts)")
    with pytest.raises(Exception):
        s.probe.wait(0)
    return s
