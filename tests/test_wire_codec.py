"""Trace wire codec on the host (no GPU): the reference encoder followed by the pool decoder gives
back every byte, the encoded size is what the format's rules say, and wire buffers that do not
parse are refused."""
import ctypes

import numpy as np
import pytest

from tachikoma_amd import _lib
from tests import wire_cases as wc

LIB = _lib.load()
INVALID_ARG = -1   # TK_ERR_INVALID_ARG (include/tachikoma.h)
NAMES = sorted(wc.contents(1, np.random.default_rng(0)))


def _encode(records, diffs, offs, total):
    recs = wc.wire_records(records, diffs, offs)
    src = wc.image_of(records, offs, total)
    bound = LIB.tk_wire_bound(recs, len(records))
    assert bound > 0, LIB.tk_last_error()
    wire = np.zeros(bound, np.uint8)
    n = LIB.tk_wire_encode_host(recs, len(records), wc.ptr(src), total, wc.ptr(wire), bound)
    assert n > 0, LIB.tk_last_error()
    return recs, src, wire, n


def _decode(recs, n_recs, wire, n, offs, records, total, threads=0):
    # the wire bytes alone, in a buffer of exactly that size
    exact = np.ascontiguousarray(wire[:n]).copy()
    out = wc.image_of([np.zeros_like(r) for r in records], offs, total)
    rc = LIB.tk_wire_decode(recs, n_recs, wc.ptr(exact), n, wc.ptr(out), total, threads)
    return rc, out


@pytest.mark.parametrize("n", wc.SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_roundtrip_is_bit_exact(name, n):
    """Every content on every size, records at odd image offsets with guard bytes between them:
    the decoded image equals the source image (guards included: nothing written outside a record),
    and the encoder chose the widths the format prescribes (size restated in NumPy)."""
    records, diffs = wc.contents(n, np.random.default_rng(n))[name]
    offs, total = wc.layout(records)
    assert all(o % 2 == 1 for o in offs[:1])
    recs, src, wire, nbytes = _encode(records, diffs, offs, total)
    assert nbytes == wc.expected_bytes(records, diffs)
    rc, out = _decode(recs, len(records), wire, nbytes, offs, records, total)
    assert rc == 0, LIB.tk_last_error()
    assert np.array_equal(out, src)


def test_width_boundaries():
    """One full block per range: 0 -> width 0, 255 -> 1, 256 -> 2, 65535 -> 2, 65536 -> 3,
    2^24 - 1 -> 3, 2^24 -> 4, INT_MIN with INT_MAX -> 4 (not a wrapped range)."""
    rng = np.random.default_rng(1)
    for width_of, rg in [(0, 0), (1, 255), (2, 256), (2, 65535), (3, 65536), (3, 2 ** 24 - 1), (4, 2 ** 24),
                         (4, 2 ** 32 - 1)]:
        lo = wc.INT_MIN if rg == 2 ** 32 - 1 else -1234
        r = wc._span(256, lo, rg, rng)
        offs, total = wc.layout([r])
        _, _, wire, nbytes = _encode([r], [0], offs, total)
        assert nbytes == 64 + 64 * ((32 + width_of * 256 + 63) // 64), (rg, nbytes)
        assert wire[64 + 16] == width_of          # table | base (16) | width ...
        assert wire[64:68].view(np.int32)[0] == lo


def test_random_full_range_costs_at_most_3_percent():
    """Data that does not narrow: every block takes the raw escape and the overhead is the 5 header
    bytes per block, the rounding of a 64-block segment to 64 B and 4 table bytes per segment.
    The bound is a ratio, so it is taken where the per-record constants (one 64-byte table line,
    one 64-byte rounding) are amortised: a record of 2^20 elements; the small sizes are held to
    the exact size above."""
    n = 1 << 20
    r = np.random.default_rng(5).integers(wc.INT_MIN, wc.INT_MAX + 1, n, dtype=np.int64).astype(np.int32)
    offs, total = wc.layout([r])
    recs, src, wire, nbytes = _encode([r], [0], offs, total)
    assert nbytes <= 1.03 * 4 * n, nbytes / (4 * n)
    assert LIB.tk_wire_bound(recs, 1) <= 1.03 * 4 * n
    for threads in (1, 0):
        rc, out = _decode(recs, 1, wire, nbytes, offs, [r], total, threads)
        assert rc == 0 and np.array_equal(out, src)


def test_multi_segment_chain():
    """Three records differenced in a chain, two full segments and a short one each: the decoder
    works through (segment, chain member) in order on several threads."""
    n = 2 * wc.SEG + 300
    records, diffs = wc.contents(n, np.random.default_rng(9))["diff_chain"]
    offs, total = wc.layout(records)
    recs, src, wire, nbytes = _encode(records, diffs, offs, total)
    assert nbytes == wc.expected_bytes(records, diffs)
    assert nbytes < 0.55 * sum(4 * len(r) for r in records)   # 3 bytes, then 1 byte, then 1 byte per element
    rc, out = _decode(recs, 3, wire, nbytes, offs, records, total)
    assert rc == 0 and np.array_equal(out, src)


def test_broken_wire_buffers_are_refused():
    """A truncated table, a truncated payload, a table entry past the buffer and a width code above
    4 all fail with TK_ERR_INVALID_ARG; the decoder is given exactly the bytes it may read."""
    records, diffs = wc.contents(3 * 256 + 17, np.random.default_rng(2))["diff_chain"]
    n = 2 * wc.SEG + 300
    records = [np.resize(r, n) for r in records]
    offs, total = wc.layout(records)
    recs, src, wire, nbytes = _encode(records, diffs, offs, total)
    table = 64   # 9 segments

    def refused(w, nb):
        rc, _ = _decode(recs, 3, w, nb, offs, records, total)
        return rc == INVALID_ARG
    assert refused(wire, 0) and refused(wire, 4) and refused(wire, table - 1)
    assert refused(wire, table) and refused(wire, nbytes - 64)
    bad = wire.copy()
    bad[4:8].view(np.uint32)[0] = nbytes // 64       # segment 1 starts at the end of the buffer
    assert refused(bad, nbytes)
    bad = wire.copy()
    bad[8:12].view(np.uint32)[0] = 0xFFFFFFFF
    assert refused(bad, nbytes)
    bad = wire.copy()
    bad[table + 256 + 3] = 5                          # width of block 3 of the first segment
    assert refused(bad, nbytes)
    # the segment that lies last claims every block raw: longer than the buffer holds
    last = int(np.argmax(wire[:36].view(np.uint32)))
    start = int(wire[4 * last:4 * last + 4].view(np.uint32)[0]) * 64
    nb = 2 if last % 3 == 2 else 64                   # per record: two full segments and a short one
    bad = wire.copy()
    bad[table + start + (4 * nb + 15) // 16 * 16:][:nb] = 4
    assert refused(bad, nbytes)
    # records that do not fit the image, or a difference against a record of another size
    r2 = wc.wire_records(records, diffs, offs)
    r2[2].n_elems += 1
    assert LIB.tk_wire_bound(r2, 3) == INVALID_ARG
    r3 = wc.wire_records(records, [0, 0, 0], offs)
    r3[2].offset = total - 8
    rc = LIB.tk_wire_decode(r3, 3, wc.ptr(wire), nbytes, wc.ptr(src.copy()), total, 0)
    assert rc == INVALID_ARG
    # the intact buffer still decodes
    rc, out = _decode(recs, 3, wire, nbytes, offs, records, total)
    assert rc == 0 and np.array_equal(out, src)


def test_pool_size_follows_affinity():
    import os
    n = LIB.tk_wire_threads()
    env = os.environ.get("TK_WIRE_THREADS")
    if env and env.isdigit() and 1 <= int(env) <= 16:
        assert n == int(env)
    else:
        assert n == min(16, len(os.sched_getaffinity(0)))
