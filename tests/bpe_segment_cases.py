"""Inputs and a lane-level emulation for the per-segment-minimum BPE merge
schedule (csrc/bpe_kernels.cuh, bpe_merge_lanes<true>).

Plain helper module (no tests here): tests/test_bpe_segment_min_cpu.py runs
the emulation against BPERef on the CPU, tests/test_gpu_bpe_segment_min.py
feeds the same texts to the real kernels.
"""

from __future__ import annotations

import numpy as np

from aigw.ops.bpe_ref import CHUNK, byte_class, segment_starts

INF = 2 ** 31 - 1  # INT_MAX, the kernel's "no pair" rank

_LETTERS = b"etaoinshr"


def letters(n: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    return bytes(_LETTERS[int(i)] for i in rng.integers(0, len(_LETTERS), n))


def group_span_65() -> bytes:
    """One request whose first group has segment starts 0,5,..,30 (one
    32-byte cell) and ends at byte 65, where the next group starts: the
    span exceeds the 64-lane window by one byte, so the last segment takes
    the chunked single-segment path while the first six are packed."""
    head = b"etaoi" + b" nshr" * 5        # segments start at 0,5,10,15,20,25
    last = b" " + letters(34, 9)          # starts at 30, ends at 65
    return head + last + b" tail end"


# '#' occurs in no merge (the table pairs letters, space and merged ids
# only), so the " ##" segments have pairs but none that merges
NO_MERGE_BETWEEN = b" the ## the ##x the"

SINGLE_GROUP_TEXTS = {
    "equal_minima": b" the the the the the",
    "depths_0_to_many": b"a seventeen x1 of",
    "overlaps": b"aaaa aaa aa a",
    "span_65": group_span_65(),
    "no_merge_between": NO_MERGE_BETWEEN,
}

VOCAB_30 = (
    b"the", b"of", b"and", b"to", b"in", b"is", b"that", b"it", b"seventeen",
    b"aaaa", b"aaa", b"aa", b"a", b"x1", b"2024", b"hello,", b"world!",
    b"e.g.", b"ratio", b"station", b"there", b"either", b"shore", b"tenth",
    b"##", b"\n", b"into", b"90210", b"noise", b"the",
)


def seeded_200() -> list[bytes]:
    """200 texts of 1-300 bytes over a 30-word vocabulary with repeats."""
    rng = np.random.default_rng(4620)
    out = []
    for n in rng.integers(1, 301, 200):
        words = []
        size = 0
        while size < n:
            w = VOCAB_30[int(rng.integers(0, len(VOCAB_30)))]
            if rng.random() < 0.3 and words:
                w = words[-1]  # immediate repeat
            words.append(w)
            size += len(w) + 1
        out.append(b" ".join(words)[: int(n)])
    return out


def cases() -> dict:
    """name -> list of request texts."""
    out = {name: [t] for name, t in SINGLE_GROUP_TEXTS.items()}
    # behind a 13-byte first request every 32-byte cell is unaligned to
    # the byte buffer
    for name, t in SINGLE_GROUP_TEXTS.items():
        out[name + "_behind_13"] = [b"thirteen byte", t]
    out["seeded_200"] = seeded_200()
    return out


# ---------------------------------------------------------------------------
# lane-level emulation of bpe_encode_grouped_body
# ---------------------------------------------------------------------------

def merge_lanes(tok: list, myseg: list, rank_of: dict, segmented: bool):
    """Emulates bpe_merge_lanes on 64 lanes, in place on `tok` (-1 = lane
    holds no token). Returns the number of merge rounds executed."""
    lanes = range(64)
    if segmented:
        # loop-invariant: "lane - 2^k is in my segment" bits, last lane
        inseg = [[l >= (1 << k) and myseg[l - (1 << k)] == myseg[l]
                  for k in range(6)] for l in lanes]
        # (segment ids never decrease along the lanes)
        last_of = {s: l for l, s in enumerate(myseg)}
        seg_last = [last_of[s] for s in myseg]
    rounds = 0
    while True:
        active = [t >= 0 for t in tok]
        nxt, prev = [-1] * 64, [-1] * 64  # neighbouring active lanes
        seen = -1
        for l in reversed(lanes):
            nxt[l] = seen
            if active[l]:
                seen = l
        seen = -1
        for l in lanes:
            prev[l] = seen
            if active[l]:
                seen = l
        rank = [INF] * 64
        for l in lanes:
            if tok[l] >= 0 and nxt[l] >= 0 and myseg[nxt[l]] == myseg[l]:
                rank[l] = rank_of.get((tok[l], tok[nxt[l]]), INF)
        if segmented:
            v = list(rank)
            for k in range(6):  # segmented inclusive prefix-min
                up = [v[l - (1 << k)] if l >= (1 << k) else v[l] for l in lanes]
                v = [min(v[l], up[l]) if inseg[l][k] else v[l] for l in lanes]
            minrank = [v[seg_last[l]] for l in lanes]
        else:
            minrank = [min(rank)] * 64
        if all(m == INF for m in minrank):
            return rounds
        rounds += 1
        occ = [rank[l] == minrank[l] and rank[l] != INF for l in lanes]
        sel = [False] * 64
        m = list(occ)
        for l in lanes:  # greedy leftmost non-overlapping selection
            if m[l]:
                sel[l] = True
                m[l] = False
                if nxt[l] >= 0:
                    m[nxt[l]] = False
        for l in lanes:
            new = tok[l]
            if sel[l]:
                new = 256 + minrank[l]
            if prev[l] >= 0 and sel[prev[l]]:
                new = -1
            tok[l] = new


def _one_segment(data: bytes, s: int, e: int, rank_of: dict):
    ids, rounds = [], 0
    for c in range(s, e, CHUNK):
        chunk = data[c:min(c + CHUNK, e)]
        tok = list(chunk) + [-1] * (64 - len(chunk))
        rounds += merge_lanes(tok, [0] * 64, rank_of, False)
        ids.extend(t for t in tok if t >= 0)
    return ids, rounds


def encode_grouped(texts: list, rank_of: dict, segmented: bool):
    """Emulates the grouped pipeline end to end: segmentation, 32-byte-cell
    grouping, the packed window (or the chunked path) per group.
    Returns (ids per request, rounds per group, segments per group)."""
    data = b"".join(texts)
    n = len(data)
    offs, off = [], 0
    for t in texts:
        offs.append(off)
        off += len(t)
    starts = segment_starts(data, offs)
    seg_req, req = [], 0
    for s in starts:
        while req + 1 < len(texts) and s >= offs[req + 1]:
            req += 1
        seg_req.append(req)
    heads = [i for i in range(len(starts))
             if i == 0 or seg_req[i] != seg_req[i - 1] or
             ((starts[i] - offs[seg_req[i]]) >> 5) !=
             ((starts[i - 1] - offs[seg_req[i]]) >> 5)]
    out = [[] for _ in texts]
    group_rounds, group_segs = [], []
    for g, first in enumerate(heads):
        next_first = heads[g + 1] if g + 1 < len(heads) else len(starts)
        lastseg = next_first - 1
        s0 = starts[first]
        sE = starts[next_first] if next_first < len(starts) else n
        if lastseg == first:
            ids, rounds = _one_segment(data, s0, sE, rank_of)
        else:
            sL = starts[lastseg]
            include_last = (sE - s0) <= 64
            win_end = sE if include_last else sL
            assert win_end - s0 <= 64
            tok, myseg, seg = [], [], 0
            for lane in range(64):
                pos = s0 + lane
                f = False
                if pos < win_end:
                    b, pb = data[pos], data[pos - 1] if pos else 0
                    f = pos == s0 or b == 0x20 or (
                        byte_class(b) != byte_class(pb) and pb != 0x20)
                seg += f
                tok.append(data[pos] if pos < win_end else -1)
                myseg.append(seg)
            rounds = merge_lanes(tok, myseg, rank_of, segmented)
            ids = [t for t in tok if t >= 0]
            if not include_last:
                tail, r2 = _one_segment(data, sL, sE, rank_of)
                ids += tail
                rounds += r2
        out[seg_req[first]].extend(ids)
        group_rounds.append(rounds)
        group_segs.append(next_first - first)
    return out, group_rounds, group_segs
