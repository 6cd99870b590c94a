"""Shared cases of the 1-byte trace wire codec tests (host and device): (predecessor, record) pairs
that a clamp does and does not reproduce, plain 1-byte records, an image builder with odd record
offsets for records of any kind, and a NumPy restatement of the encoded size (csrc/tk_wire.h)."""
import numpy as np

from tachikoma_amd import _lib
from tests import wire_cases as wc

SIZES = [1, 15, 16, 17, 255, 256, 257, 3 * 256 + 17, 2 * 16384 + 300]
KINDS = {1: np.int8, 2: np.uint8}     # tk_wire_record.kind of the 1-byte records
BLOCK, SEG = wc.BLOCK, wc.SEG


def kind_of(r):
    return {np.dtype(np.int32): 0, np.dtype(np.int8): 1, np.dtype(np.uint8): 2}[r.dtype]


def _full(n, dt, rng):
    """n values over the dtype's whole range, both of its ends in every block (where it has two
    elements)."""
    lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
    v = rng.integers(lo, hi + 1, n, dtype=np.int64)
    for b in range(0, n, BLOCK):
        v[b] = lo
        if min(n, b + BLOCK) - b > 1:
            v[b + 1] = hi
    return v.astype(dt)


def contents(n, kind, rng):
    """name -> (records, diff flags): diff 1 is a record clamp-predicted from the one before it."""
    dt = KINDS[kind]
    lo, hi = int(np.iinfo(dt).min), int(np.iinfo(dt).max)
    prev = _full(n, dt, rng)
    c = {
        # only the lower bound is hit (the upper one is the dtype's)
        "relu": ([prev, np.clip(prev, lo + 128, hi).astype(dt)], [0, 1]),
        "both_bounds": ([prev, np.clip(prev, lo + 60, hi - 70).astype(dt)], [0, 1]),
        "identity": ([prev, prev.copy()], [0, 1]),
        # bounds at -128 / 127 and at 0 / 255: both present in every block of prev
        "dtype_ends": ([prev, np.clip(prev, lo, hi).astype(dt)], [0, 1]),
        "constant_plain": ([np.full(n, lo + 17, dt)], [0]),
        "random_plain": ([rng.integers(lo, hi + 1, n, dtype=np.int64).astype(dt)], [0]),
    }
    # the first block holds nothing the bounds touch; the others are clamped on both sides
    quiet = prev.copy()
    quiet[:BLOCK] = rng.integers(lo + 90, hi - 90, min(n, BLOCK), dtype=np.int64).astype(dt)
    c["block_unclamped"] = ([quiet, np.clip(quiet, lo + 60, hi - 70).astype(dt)], [0, 1])
    # one element off by one, last in the (usually short) final block: only that block may go raw
    off = np.clip(prev, lo + 60, hi - 70).astype(dt)
    off[-1] = off[-1] + 1 if off[-1] == lo + 60 else off[-1] - 1
    c["off_by_one"] = ([prev, off], [0, 1])
    if kind == 2:
        # values above 127 on both sides of bounds that are above 127 themselves: a signed compare
        # orders all of them below 0 .. 127 and gets min, max and the clamp wrong
        high = rng.integers(100, 256, n, dtype=np.int64).astype(dt)
        high[::2] = rng.integers(129, 150, len(high[::2]), dtype=np.int64).astype(dt)
        high[1::2] = rng.integers(221, 256, len(high[1::2]), dtype=np.int64).astype(dt)
        if n > 2:
            high[2::5] = rng.integers(100, 256, len(high[2::5]), dtype=np.int64).astype(dt)
        c["u8_above_127"] = ([high, np.clip(high, 150, 220).astype(dt)], [0, 1])
    return c


def layout(records, first=3, gap=5):
    """Odd image offsets for records of any element size."""
    offs, at = [], first
    for r in records:
        offs.append(at)
        at += r.nbytes + gap
    return offs, at + 9


def wire_records(records, diffs, offs):
    arr = (_lib.tk_wire_record * len(records))()
    for i, r in enumerate(records):
        arr[i].offset, arr[i].n_elems, arr[i].diff, arr[i].kind = offs[i], len(r), diffs[i], kind_of(r)
    return arr


def image_of(records, offs, total, fill=0xA5):
    img = np.full(total, fill, np.uint8)
    for r, o in zip(records, offs):
        img[o:o + r.nbytes] = r.view(np.uint8)
    return img


def block_widths(records, diffs):
    """Per record, the width of every block by the format's rules (segments do not matter: they are
    whole blocks).  int32 records by tests/wire_cases.py's rule; a plain 1-byte block is 0 when
    constant, else 1; a clamp-predicted one is 0 when clamp(prev block, min, max) gives the block
    (min and max the block's own, in the record's dtype), else 1."""
    out = []
    for i, r in enumerate(records):
        ws = []
        for b in range(0, len(r), BLOCK):
            blk = r[b:b + BLOCK]
            if r.dtype == np.int32:
                v = blk.astype(np.int64)
                if diffs[i]:
                    v = ((v - records[i - 1][b:b + BLOCK].astype(np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31
                rg = int(v.max() - v.min())
                ws.append(0 if rg == 0 else 1 if rg <= 0xFF else 2 if rg <= 0xFFFF else 3 if rg <= 0xFFFFFF else 4)
            elif diffs[i]:
                ws.append(0 if np.array_equal(np.clip(records[i - 1][b:b + BLOCK], blk.min(), blk.max()), blk) else 1)
            else:
                ws.append(0 if blk.min() == blk.max() else 1)
        out.append(ws)
    return out


def expected_bytes(records, diffs):
    """Wire size: the table, then per segment of 64 blocks the header (bases and widths, each
    padded to 16 B) and width * count bytes per block, rounded to 64 B."""
    n_seg, total = 0, 0
    for r, ws in zip(records, block_widths(records, diffs)):
        for s in range(0, len(ws), SEG // BLOCK):
            seg_w = ws[s:s + SEG // BLOCK]
            nb = len(seg_w)
            size = wc._a(4 * nb, 16) + wc._a(nb, 16)
            for j, w in enumerate(seg_w):
                size += w * min(BLOCK, len(r) - (s + j) * BLOCK)
            total += wc._a(size, 64)
            n_seg += 1
    return wc._a(4 * n_seg, 64) + total


def stated_widths(wire, records):
    """Per record, the widths its segments state in a wire buffer (segments may lie in any order)."""
    seg_n = [(i, min(SEG, len(r) - s)) for i, r in enumerate(records) for s in range(0, len(r), SEG)]
    table = wc._a(4 * len(seg_n), 64)
    starts = wire[:4 * len(seg_n)].view(np.uint32)
    out = [[] for _ in records]
    for (i, n), st in zip(seg_n, starts):
        nb = (n + BLOCK - 1) // BLOCK
        at = table + int(st) * 64 + wc._a(4 * nb, 16)
        out[i] += [int(w) for w in wire[at:at + nb]]
    return out


parsed_bytes = wc.parsed_bytes    # counts elements and stated widths: the same for every kind
ptr = wc.ptr
