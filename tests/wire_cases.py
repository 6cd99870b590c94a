"""Shared cases of the trace wire codec tests (host and device): record contents that sit on every
width boundary of the format, an image builder with odd record offsets, and a NumPy restatement of
the encoded size (csrc/tk_wire.h) to hold the encoders against."""
import ctypes

import numpy as np

from tachikoma_amd import _lib

SIZES = [1, 255, 256, 257, 3 * 256 + 17]
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
BLOCK, SEG = 256, 256 * 64


def _span(n, lo, rng_width, rng):
    """n values in [lo, lo + rng_width] with both ends present in every block of 256 (where the
    block has two elements)."""
    v = rng.integers(lo, lo + rng_width + 1, n, dtype=np.int64)
    for b in range(0, n, BLOCK):
        v[b] = lo
        if min(n, b + BLOCK) - b > 1:
            v[b + 1] = lo + rng_width
    return v.astype(np.int32)


def contents(n, rng):
    """name -> (list of int32 records, list of diff flags)."""
    c = {
        "constant": ([np.full(n, -77, np.int32)], [0]),
        "range_255": ([_span(n, -100, 255, rng)], [0]),
        "range_256": ([_span(n, -100, 256, rng)], [0]),
        "range_65535": ([_span(n, 1000, 65535, rng)], [0]),
        "range_65536": ([_span(n, 1000, 65536, rng)], [0]),
        "range_2p24m1": ([_span(n, -5_000_000, 2 ** 24 - 1, rng)], [0]),
        "range_2p24": ([_span(n, -5_000_000, 2 ** 24, rng)], [0]),
        "int_min_max": ([_span(n, INT_MIN, 2 ** 32 - 1, rng)], [0]),
        "random_full": ([rng.integers(INT_MIN, INT_MAX + 1, n, dtype=np.int64).astype(np.int32)], [0]),
        # a - prev wraps: INT_MAX - INT_MIN = -1 (mod 2^32)
        "diff_wraps": ([np.full(n, INT_MIN, np.int32), np.full(n, INT_MAX, np.int32)], [0, 1]),
    }
    # a convolution's accumulators, then the same plus a per-channel constant, twice
    a, b = _span(n, -60000, 120000, rng), np.arange(n, dtype=np.int32) // 7 * 3 - 11
    c["diff_chain"] = ([a, a + b, a + b + b], [0, 1, 1])
    return c


def layout(records, first=3, gap=5):
    """Odd image offsets: record i at first + sum of sizes + i * gap (first, gap odd / odd)."""
    offs, at = [], first
    for r in records:
        offs.append(at)
        at += 4 * len(r) + gap
    return offs, at + 9


def wire_records(records, diffs, offs):
    arr = (_lib.tk_wire_record * len(records))()
    for i, r in enumerate(records):
        arr[i].offset, arr[i].n_elems, arr[i].diff = offs[i], len(r), diffs[i]
    return arr


def image_of(records, offs, total, fill=0xA5):
    img = np.full(total, fill, np.uint8)
    for r, o in zip(records, offs):
        img[o:o + 4 * len(r)] = r.view(np.uint8)
    return img


def _a(x, m):
    return (x + m - 1) // m * m


def expected_bytes(records, diffs):
    """Wire size by the format's rules: the table, then per segment of 64 blocks the header (bases
    and widths, each padded to 16 B) and width * count bytes per block, rounded to 64 B."""
    n_seg, total = 0, 0
    for i, r in enumerate(records):
        v = r.astype(np.int64)
        if diffs[i]:
            v = ((v - records[i - 1].astype(np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31   # int32 wrap
        for s in range(0, len(v), SEG):
            seg = v[s:s + SEG]
            nb = (len(seg) + BLOCK - 1) // BLOCK
            size = _a(4 * nb, 16) + _a(nb, 16)
            for b in range(0, len(seg), BLOCK):
                blk = seg[b:b + BLOCK]
                rng = int(blk.max() - blk.min())
                w = 0 if rng == 0 else 1 if rng <= 0xFF else 2 if rng <= 0xFFFF else 3 if rng <= 0xFFFFFF else 4
                size += w * len(blk)
            total += _a(size, 64)
            n_seg += 1
    return _a(4 * n_seg, 64) + total


def parsed_bytes(wire, records):
    """Wire size read back from a wire buffer: the table plus every segment's header and block
    payloads by the widths it states, each segment rounded to 64 B (segments may lie in any order)."""
    seg_n = [min(SEG, len(r) - s) for r in records for s in range(0, len(r), SEG)]
    table = _a(4 * len(seg_n), 64)
    starts = wire[:4 * len(seg_n)].view(np.uint32)
    total = table
    for n, st in zip(seg_n, starts):
        nb = (n + BLOCK - 1) // BLOCK
        at = table + int(st) * 64 + _a(4 * nb, 16)
        widths = wire[at:at + nb].astype(np.int64)
        counts = np.minimum(BLOCK, n - BLOCK * np.arange(nb))
        total += _a(_a(4 * nb, 16) + _a(nb, 16) + int((widths * counts).sum()), 64)
    return total


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data)
