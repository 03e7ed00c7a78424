"""CPU: the byte-space group-head rule of front_flags_kernel
(csrc/admission_front_kernels.cuh) against the segment-space rule of
group_flags_count_kernel (csrc/bpe_kernels.cuh).

Segment space: segment j heads a group iff j == 0, it belongs to another
request than segment j-1, or its start lies in another 32-byte cell
(relative to the request start) than the start of segment j-1.
Byte space: a segment start at byte i of request r heads a group iff no
other segment start lies in [off[r] + 32*((i - off[r]) >> 5), i).

heads_tiled() additionally walks the bytes the way the kernel does: one
256-byte tile at a time, seeing only the tile, the 32 bytes before it and
the offsets, with the segment flags of the look-back recomputed."""

from bisect import bisect_right

import numpy as np
import pytest

from aigw.ops.bpe_ref import byte_class, segment_starts

TILE, BACK = 256, 32


def offsets(texts):
    offs, off = [], 0
    for t in texts:
        offs.append(off)
        off += len(t)
    return offs


def heads_segment_space(data: bytes, offs: list) -> list:
    """(ghead, seg_start, seg_req) as the seven-kernel pipeline builds them."""
    starts = segment_starts(data, offs)
    seg_req = [bisect_right(offs, s) - 1 for s in starts]  # upper_bound - 1
    ghead = [j for j in range(len(starts))
             if j == 0 or seg_req[j] != seg_req[j - 1] or
             ((starts[j] - offs[seg_req[j]]) >> 5) !=
             ((starts[j - 1] - offs[seg_req[j]]) >> 5)]
    return ghead, starts, seg_req


def heads_byte_space(data: bytes, offs: list) -> list:
    starts = segment_starts(data, offs)
    is_start = bytearray(len(data))
    for s in starts:
        is_start[s] = 1
    ghead = []
    for j, i in enumerate(starts):
        off = offs[bisect_right(offs, i) - 1]
        cell = off + 32 * ((i - off) >> 5)
        if not any(is_start[cell:i]):
            ghead.append(j)
    return ghead


def _class_start(b: int, p: int) -> bool:
    return b == 0x20 or (byte_class(b) != byte_class(p) and p != 0x20)


def heads_tiled(data: bytes, offs: list) -> list:
    """Byte positions of the group heads, one tile at a time."""
    n = len(data)
    heads = []
    for base in range(0, n, TILE):
        end = min(base + TILE, n)
        lo_byte = max(base - BACK, 0)
        forced = [0] * (BACK + TILE)  # window position p = byte base - 32 + p
        prev_start = -1
        for off in offs:
            if off >= end:
                break
            if off < base:
                prev_start = max(prev_start, off)
            if off >= lo_byte:
                forced[off - (base - BACK)] = 1
        flag = [0] * (BACK + TILE)
        for p in range(BACK + TILE):
            i = base - BACK + p
            if p < BACK and (base == 0 or p == 0):
                continue  # no byte there / a predecessor only
            if i >= n:
                break
            flag[p] = int(i == 0 or forced[p] or
                          _class_start(data[i], data[i - 1]))
        rs = prev_start
        for t in range(end - base):
            q = BACK + t
            i = base + t
            if forced[q]:
                rs = i
            if flag[q]:
                k = (i - max(rs, 0)) & 31
                assert q - k >= 1
                if not any(flag[q - k:q]):
                    heads.append(i)
    return heads


_WORDS = (b"a", b"b", b"I", b"x", b"the", b"of", b"seventeen", b"42", b"7",
          b"e.g.", b"\n", b"--", b"\xc3\xa9t\xc3\xa9")


def _text(rng, n: int) -> bytes:
    """n bytes mixing single-letter words, long letter runs, digits,
    punctuation and runs of spaces."""
    kind = int(rng.integers(0, 4))
    if kind == 0:    # single-letter words: up to 16 segments per 32-byte cell
        body = b" ".join(_WORDS[int(i)] for i in rng.integers(0, 4, n))
    elif kind == 1:  # long letter runs: cells without any segment start
        body = b" ".join(bytes(rng.integers(97, 123, int(m)).astype(np.uint8))
                         for m in rng.integers(20, 200, n // 20 + 1))
    elif kind == 2:  # class changes, double spaces
        body = b"".join(_WORDS[int(i)] + b" " * int(s) for i, s in
                        zip(rng.integers(0, len(_WORDS), n),
                            rng.integers(0, 3, n)))
    else:            # any byte
        body = bytes(rng.integers(0, 256, n).astype(np.uint8))
    return body[:n]


def _batch(rng) -> list:
    texts = []
    for _ in range(int(rng.integers(1, 12))):
        roll = rng.random()
        if roll < 0.15:
            texts += [b""] * int(rng.integers(1, 4))  # empty, alone or a run
        elif roll < 0.4:
            # end the text 0-3 bytes around the next multiple of 256
            size = sum(len(t) for t in texts)
            target = (size // 256 + 1) * 256 + int(rng.integers(-3, 4))
            texts.append(_text(rng, max(target - size, 1)))
        else:
            texts.append(_text(rng, int(rng.integers(1, 400))))
    if rng.random() < 0.3:
        texts.append(b"")  # trailing empty text: its offset equals n
    if not any(texts):
        texts.append(_text(rng, 33))
    return texts


@pytest.mark.parametrize("seed", range(40))
def test_byte_space_rule_matches_segment_space(seed):
    rng = np.random.default_rng(7100 + seed)
    for _ in range(5):
        texts = _batch(rng)
        data, offs = b"".join(texts), offsets(texts)
        ghead, starts, _ = heads_segment_space(data, offs)
        assert heads_byte_space(data, offs) == ghead
        assert heads_tiled(data, offs) == [starts[j] for j in ghead]


def test_batches_cover_what_they_claim():
    """The generator really produces the mixes the rule has to survive."""
    rng = np.random.default_rng(7100)
    seen = {"dense_cell": False, "empty_run": False, "trailing_empty": False,
            "unaligned_off": False, "straddle_256": False, "bare_cell": False}
    for _ in range(200):
        texts = _batch(rng)
        data, offs = b"".join(texts), offsets(texts)
        ghead, starts, _ = heads_segment_space(data, offs)
        sizes = np.diff(ghead + [len(starts)])
        seen["dense_cell"] |= bool((sizes >= 12).any())
        seen["bare_cell"] |= any(b - a > 64 for a, b in zip(starts, starts[1:]))
        seen["empty_run"] |= any(a == b == c for a, b, c in
                                 zip(offs, offs[1:], offs[2:]))
        seen["trailing_empty"] |= offs[-1] == len(data)
        seen["unaligned_off"] |= any(o % 32 for o in offs)
        seen["straddle_256"] |= any(0 < o < len(data) and o % 256 in (253, 254, 255, 1, 2, 3)
                                    for o in offs)
    assert all(seen.values()), seen


def test_known_small_cases():
    # 40 one-letter words: starts at 0 and at every odd byte from 1
    # ("a" then " a" ...), so cells [0,32) and [32,64)... each hold one head
    data = b" ".join([b"a"] * 40)
    ghead, starts, _ = heads_segment_space(data, [0])
    assert [starts[j] for j in ghead] == [0, 33, 65]
    assert heads_tiled(data, [0]) == [0, 33, 65]
    # the same text behind a 250-byte request: cells are relative to 250
    # and the first of them straddles byte 256
    first = b"e" * 250
    both = first + data
    want = [0, 250, 250 + 33, 250 + 65]
    assert heads_tiled(both, [0, 250]) == want
    assert heads_tiled(both, [0, 250, 250]) == want  # an empty text before it
