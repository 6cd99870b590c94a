"""Shared cases of the bias-coding tests of the trace wire (host and device): pairs [a, a + bias[c]]
over a grid of (plane, channels, samples), the contents the prediction must survive, record arrays
with addends and a NumPy restatement of the rule (csrc/tk_wire.h: the coded value of element e of a
record with an addend is rec[e] - prev[e] - addend[(e / plane) % channels], int32 wrap-around)."""
import ctypes

import numpy as np

from tachikoma_amd import _lib
from tests import wire_cases as wc

# (plane, channels, samples): dense (plane 1), planes below a lane's 16 elements, the 7x7 and 14x14
# planes where every block straddles, 9x9, a plane of exactly one block, one element more, and a
# plane longer than a segment (the second segment starts mid-plane)
GRID = [(1, 10, 5), (3, 5, 40), (7, 24, 3), (49, 24, 2), (81, 8, 3), (196, 4, 3), (256, 3, 2), (257, 3, 2),
        (16385, 2, 1)]


def channel_of(n, plane, channels):
    return (np.arange(n, dtype=np.int64) // plane) % channels


def wrap(v):
    """int64 -> int32 with wrap-around."""
    return ((np.asarray(v, np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)


def bias_pair(plane, channels, samples, rng, bias=None):
    """A convolution's accumulators and the same plus bias[c]: (records, diffs, addends)."""
    n = plane * channels * samples
    a = rng.integers(-60000, 60001, n, dtype=np.int64).astype(np.int32)
    if bias is None:
        bias = (rng.permutation(channels).astype(np.int64) * 1013 - 30000).astype(np.int32)   # all distinct
    b = wrap(a.astype(np.int64) + bias.astype(np.int64)[channel_of(n, plane, channels)])
    return [a, b], [0, 1], [None, (plane, channels, bias)]


def cases(rng):
    """name -> (records, diffs, addends, flat): `flat` lists the records that are true bias_adds of
    their predecessor (every block of them must be coded at width 0)."""
    c = {}
    for plane, channels, samples in GRID:
        c[f"grid_{plane}_{channels}_{samples}"] = bias_pair(plane, channels, samples, rng) + ([1],)
    # a length that is no multiple of the block: 3 * 256 + 17 elements of a dense record
    c["ragged"] = bias_pair(1, 157, 5, rng) + ([1],)
    assert len(c["ragged"][0][0]) == 3 * 256 + 17
    # addends at both ends of int32: a + bias wraps, and so does the difference
    ends = np.array([wc.INT_MIN, wc.INT_MAX, -1, 0, wc.INT_MAX, wc.INT_MIN], np.int32)
    c["addend_ends"] = bias_pair(49, 6, 4, rng, ends) + ([1],)
    # the prediction fails everywhere: a second record of full-range noise
    recs, diffs, adds = bias_pair(49, 24, 2, rng)
    recs[1] = rng.integers(wc.INT_MIN, wc.INT_MAX + 1, len(recs[0]), dtype=np.int64).astype(np.int32)
    c["prediction_fails"] = (recs, diffs, adds, [])
    # a chain of three, each the bias_add of the one before
    recs, diffs, adds = bias_pair(196, 4, 3, rng)
    bias2 = np.array([5, -70000, wc.INT_MAX, 12], np.int32)
    recs.append(wrap(recs[1].astype(np.int64) + bias2.astype(np.int64)[channel_of(len(recs[1]), 196, 4)]))
    c["chain_of_three"] = (recs, diffs + [1], adds + [(196, 4, bias2)], [1, 2])
    # more than one segment with a plane below a block: segments start at any channel and position
    c["segments_49"] = bias_pair(49, 24, 30, rng) + ([1],)
    return c


def wire_records(records, diffs, addends, offs, addend_ptrs=None):
    """(the record array, the addend array beside it): a record with an addend is of kind 3 and its
    entry of the addend array holds plane, channels and the pointer, from `addend_ptrs` (record index
    -> address) or, by default, the host arrays of `addends` (which the caller keeps alive)."""
    arr = wc.wire_records(records, diffs, offs)
    ads = (_lib.tk_wire_addend * len(records))()
    for i, ad in enumerate(addends):
        if ad is None:
            continue
        arr[i].kind = 3
        ads[i].plane, ads[i].channels = ad[0], ad[1]
        ads[i].addend = addend_ptrs[i] if addend_ptrs is not None else ad[2].ctypes.data
    return arr, ads


def coded_values(records, diffs, addends, i):
    """The coded values of record i as int64 in int32 range."""
    v = records[i].astype(np.int64)
    if diffs[i]:
        v = v - records[i - 1].astype(np.int64)
    if addends[i] is not None:
        plane, channels, vec = addends[i]
        v = v - vec.astype(np.int64)[channel_of(len(v), plane, channels)]
    return wrap(v).astype(np.int64)


def expected_bytes(records, diffs, addends):
    """Wire size by the format's rules, as wire_cases.expected_bytes, with the addend subtracted."""
    n_seg, total = 0, 0
    for i in range(len(records)):
        v = coded_values(records, diffs, addends, i)
        for s in range(0, len(v), wc.SEG):
            seg = v[s:s + wc.SEG]
            nb = (len(seg) + wc.BLOCK - 1) // wc.BLOCK
            size = wc._a(4 * nb, 16) + wc._a(nb, 16)
            for b in range(0, len(seg), wc.BLOCK):
                blk = seg[b:b + wc.BLOCK]
                rng = int(blk.max() - blk.min())
                w = 0 if rng == 0 else 1 if rng <= 0xFF else 2 if rng <= 0xFFFF else 3 if rng <= 0xFFFFFF else 4
                size += w * len(blk)
            total += wc._a(size, 64)
            n_seg += 1
    return wc._a(4 * n_seg, 64) + total


def widths_of(wire, records, i):
    """The widths the wire buffer states for every block of record i (segments of a record follow
    each other in the table, records in order)."""
    seg_n = [(r, min(wc.SEG, len(x) - s)) for r, x in enumerate(records) for s in range(0, len(x), wc.SEG)]
    table = wc._a(4 * len(seg_n), 64)
    starts = wire[:4 * len(seg_n)].view(np.uint32)
    out = []
    for (r, n), st in zip(seg_n, starts):
        if r != i:
            continue
        nb = (n + wc.BLOCK - 1) // wc.BLOCK
        at = table + int(st) * 64 + wc._a(4 * nb, 16)
        out += [int(w) for w in wire[at:at + nb]]
    return out
