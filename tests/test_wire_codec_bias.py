"""Bias coding of the trace wire on the host (no GPU): a bias_add record coded as its predecessor
plus a per-channel addend.  The reference encoder followed by the pool decoder gives back every
byte whatever the addend predicts, the encoded size is what the rule says (restated in NumPy), a
true bias_add record costs its headers alone, and the entry points of the packed trace files refuse
a record with an addend."""
import ctypes

import numpy as np
import pytest

from tachikoma_amd import _lib
from tests import wire_cases as wc
from tests import wire_cases_bias as wb

LIB = _lib.load()
INVALID_ARG, UNSUPPORTED = -1, -2   # include/tachikoma.h
NAMES = sorted(wb.cases(np.random.default_rng(0)))


def _roundtrip(records, diffs, addends, first=3, gap=5, threads=0):
    offs, total = wc.layout(records, first, gap)
    recs, ads = wb.wire_records(records, diffs, addends, offs)
    src = wc.image_of(records, offs, total)
    bound = LIB.tk_wire_bound(recs, len(records))
    assert bound > 0, LIB.tk_last_error()
    wire = np.zeros(bound, np.uint8)
    n = LIB.tk_wire_encode_host_bias(recs, ads, len(records), wc.ptr(src), total, wc.ptr(wire), bound)
    assert n > 0, LIB.tk_last_error()
    exact = wire[:n].copy()   # the wire bytes alone, in a buffer of exactly that size
    out = wc.image_of([np.zeros_like(r) for r in records], offs, total)
    rc = LIB.tk_wire_decode_bias(recs, ads, len(records), wc.ptr(exact), n, wc.ptr(out), total, threads)
    assert rc == 0, LIB.tk_last_error()
    assert np.array_equal(out, src)   # guard bytes included: nothing written outside a record
    return wire, n


@pytest.mark.parametrize("layout", [(3, 5), (64, 0)], ids=["odd_offsets", "aligned"])
@pytest.mark.parametrize("name", NAMES)
def test_roundtrip_size_and_flat_blocks(name, layout):
    """Every case, records at odd image offsets (unaligned sources) and at aligned ones: the decoded
    image equals the source, the size is the rule's, every block of a true bias_add record is coded
    at width 0, and the same records without the addend cost strictly more wherever a block
    straddles a plane boundary (plane no multiple of 256)."""
    records, diffs, addends, flat = wb.cases(np.random.default_rng(7))[name]
    wire, n = _roundtrip(records, diffs, addends, *layout)
    assert n == wb.expected_bytes(records, diffs, addends) == wc.parsed_bytes(wire, records)
    for i in flat:
        widths = wb.widths_of(wire, records, i)
        assert len(widths) == sum((min(wc.SEG, len(records[i]) - s) + wc.BLOCK - 1) // wc.BLOCK
                                  for s in range(0, len(records[i]), wc.SEG))
        assert not any(widths), (name, i, widths)
    plain = [None] * len(records)
    _, n_plain = _roundtrip(records, diffs, plain, *layout)
    assert n_plain == wc.expected_bytes(records, diffs)
    if flat and any(ad is not None and ad[0] % wc.BLOCK for ad in addends):
        assert n_plain > n, (name, n_plain, n)


def test_any_addend_round_trips():
    """The addend is a predictor, not a fact: values that have nothing to do with the data (and a
    plane and channel count that are not the record's) still round-trip, on one thread and on the
    pool, at whatever width the blocks then need."""
    rng = np.random.default_rng(11)
    records, diffs, _ = wb.bias_pair(49, 24, 20, rng)
    junk = rng.integers(wc.INT_MIN, wc.INT_MAX + 1, 13, dtype=np.int64).astype(np.int32)
    addends = [None, (37, 13, junk)]
    for threads in (1, 0):
        wire, n = _roundtrip(records, diffs, addends, threads=threads)
        assert n == wb.expected_bytes(records, diffs, addends)


def test_misplaced_addends_are_refused():
    """A bias-coded record (kind 3) that is not differenced, follows a 1-byte record, or whose addend
    entry has no pointer or a plane or channel count below 1, is refused."""
    rng = np.random.default_rng(3)
    records, diffs, addends = wb.bias_pair(7, 24, 3, rng)
    offs, total = wc.layout(records)
    src = wc.image_of(records, offs, total)

    def encode(mutate):
        recs, ads = wb.wire_records(records, diffs, addends, offs)
        mutate(recs, ads)
        bound = 2 * total + 4096
        wire = np.zeros(bound, np.uint8)
        return LIB.tk_wire_encode_host_bias(recs, ads, 2, wc.ptr(src), total, wc.ptr(wire), bound)
    assert encode(lambda r, a: None) > 0
    assert encode(lambda r, a: setattr(r[1], "diff", 0)) == INVALID_ARG
    assert encode(lambda r, a: setattr(a[1], "plane", 0)) == INVALID_ARG
    assert encode(lambda r, a: setattr(a[1], "channels", -1)) == INVALID_ARG
    assert encode(lambda r, a: setattr(a[1], "addend", None)) == INVALID_ARG
    assert encode(lambda r, a: setattr(r[0], "kind", 1)) == INVALID_ARG   # a 1-byte predecessor
    # an entry beside a record of kind 0 is not read
    assert encode(lambda r, a: (setattr(r[1], "kind", 0), setattr(a[1], "addend", None))) > 0


def test_entry_points_without_addends_refuse_a_bias_coded_record():
    """tk_wire_check, tk_wire_pack_device and tk_wire_unpack_device (packed trace files keep format
    version 2) answer TK_ERR_UNSUPPORTED for a bias-coded record, before touching a buffer or the
    device, and so do the plain encoder and decoder, which are given no addends; the same records
    without the addend pass the check."""
    rng = np.random.default_rng(5)
    records, diffs, addends = wb.bias_pair(49, 24, 2, rng)
    wire, n = _roundtrip(records, diffs, addends)
    offs, total = wc.layout(records)
    recs, ads = wb.wire_records(records, diffs, addends, offs)
    exact = wire[:n].copy()
    assert LIB.tk_wire_check(recs, 2, wc.ptr(exact), n) == UNSUPPORTED
    assert b"addends" in LIB.tk_last_error()
    null = ctypes.c_void_p(0)
    ptrs = (ctypes.c_void_p * 2)()
    assert LIB.tk_wire_pack_device(recs, 2, ptrs, null, 0, null) == UNSUPPORTED
    report = (_lib.tk_wire_mismatch * 2)()
    assert LIB.tk_wire_unpack_device(recs, 2, null, 0, ptrs, 0, report, null) == UNSUPPORTED
    out = np.zeros(total, np.uint8)
    assert LIB.tk_wire_decode(recs, 2, wc.ptr(exact), n, wc.ptr(out), total, 1) == UNSUPPORTED
    assert LIB.tk_wire_encode_host(recs, 2, wc.ptr(out), total, wc.ptr(wire), len(wire)) == UNSUPPORTED
    assert LIB.tk_wire_encode_device(recs, 2, ptrs, null, 0, null) == UNSUPPORTED
    assert LIB.tk_wire_bound(recs, 2) == len(wire)   # the size does not depend on the addend
    plain_wire, plain_n = _roundtrip(records, diffs, [None, None])
    plain, _ = wb.wire_records(records, diffs, [None, None], offs)
    assert LIB.tk_wire_check(plain, 2, wc.ptr(plain_wire[:plain_n].copy()), plain_n) == 0
