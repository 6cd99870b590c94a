"""Packed trace files of format version 3 on the host (no GPU): the bias coding of the wire on disk.
pack_trace(bias=True) marks exactly the true bias_add records of the shared bias cases, the file
unpacks to the version-1 bytes, its wire has the size the format's rules give and costs headers
alone for the marked records; tk_wire_check_bias, the gate of the device decoder, accepts what
tk_wire_encode_host_bias writes and refuses what tk_wire_decode_bias refuses; every rule the reader
holds a coding-3 entry to is tried on a file edited at that one field; and version 2 is untouched.
The last group of tests builds its files in Python and needs no built library."""
import json
import struct

import numpy as np
import pytest

from tachikoma_amd import _lib
from tachikoma_amd import trace_format as tf
from tests import wire_cases as wc
from tests import wire_cases_bias as wb

INVALID_ARG = -1   # include/tachikoma.h
NAMES = sorted(wb.cases(np.random.default_rng(0)))


def _shaped(records, addends):
    """The case's flat records as (samples, channels, plane) arrays, (samples, channels) for plane 1."""
    plane, channels, _ = addends[1]
    samples = len(records[0]) // (plane * channels)
    shape = (samples, channels) if plane == 1 else (samples, channels, plane)
    return {f"r{i}": r.reshape(shape) for i, r in enumerate(records)}


def _v1(records, addends):
    params = {"w": np.arange(5, dtype=np.int32)}
    return tf.trace_bytes({"model": "bias_cases", "n_samples": 1}, params, _shaped(records, addends))


@pytest.mark.parametrize("name", NAMES)
def test_host_packer_marks_the_bias_records(name):
    """For grid_256_3_2 every block lies inside one plane, so version 2 already codes the record at
    width 0: there the wires are equal and version 3 is larger by its own bookkeeping alone (8
    bytes of section header, 9 of the plan entry, the addends), which the test holds it to."""
    records, diffs, addends, flat = wb.cases(np.random.default_rng(7))[name]
    v1 = _v1(records, addends)
    v3 = tf.pack_trace(v1, bias=True)
    v2 = tf.pack_trace(v1)
    pf = tf.parse_packed(v3)
    assert pf.version == tf.PACKED_BIAS_VERSION == 3
    assert [i for i, e in enumerate(pf.entries) if e.coding == tf.BIAS] == flat
    assert all(e.axis == 1 and e.diff == 1 for e in pf.entries if e.coding == tf.BIAS)
    assert tf.unpack_trace(v3) == v1
    marked = [ad if i in flat else None for i, ad in enumerate(addends)]
    assert pf.wire_size == wb.expected_bytes(records, diffs, marked)
    wire = np.frombuffer(v3, np.uint8)[pf.wire_off:pf.wire_off + pf.wire_size]
    for i in flat:
        assert not any(wb.widths_of(wire, records, i)), (name, i)
    for i in flat:   # the stored addends are the bias
        e, vec = pf.entries[i], addends[i][2]
        at = pf.addend_off + e.addend_off
        assert np.array_equal(np.frombuffer(v3, "<i4", len(vec), at), vec)
    plane = addends[1][0]
    if not flat:
        assert pf.addend_size == 0 and pf.wire_size == tf.parse_packed(v2).wire_size
    elif plane % wc.BLOCK:
        assert len(v3) < len(v2), (name, len(v3), len(v2))
    else:
        assert pf.wire_size == tf.parse_packed(v2).wire_size
        assert len(v3) <= len(v2) + 8 + len(flat) * 9 + 7 + pf.addend_size
    assert tf.trace_file_digest(v3) == tf.trace_file_digest(v1)
    s3, s1 = tf.trace_stats(v3), tf.trace_stats(v1)
    assert list(s3) == list(s1) and all(s3[k].equals(s1[k]) for k in s1)
    info = tf.packed_info(v3)
    assert info["version"] == 3 and [p.get("axis") for p in info["plan"]] == [1 if i in flat else None
                                                                              for i in range(len(records))]
    assert tf.read_trace(v3).records.keys() == tf.read_trace(v1).records.keys()


def _encoded(name="chain_of_three"):
    lib = _lib.load()
    records, diffs, addends, _ = wb.cases(np.random.default_rng(7))[name]
    offs, total = wc.layout(records)
    recs, ads = wb.wire_records(records, diffs, addends, offs)
    src = wc.image_of(records, offs, total)
    bound = lib.tk_wire_bound(recs, len(records))
    wire = np.zeros(bound, np.uint8)
    n = lib.tk_wire_encode_host_bias(recs, ads, len(records), wc.ptr(src), total, wc.ptr(wire), bound)
    assert n > 0, lib.tk_last_error()
    return records, recs, ads, addends, total, wire[:n].copy()


def _both(recs, ads, n_recs, wire, nbytes, total):
    """(tk_wire_check_bias, tk_wire_decode_bias) on a copy of exactly nbytes."""
    lib = _lib.load()
    exact = wire[:nbytes].copy()
    out = np.zeros(total, np.uint8)
    return (lib.tk_wire_check_bias(recs, ads, n_recs, wc.ptr(exact), nbytes),
            lib.tk_wire_decode_bias(recs, ads, n_recs, wc.ptr(exact), nbytes, wc.ptr(out), total, 1))


@pytest.mark.parametrize("name", NAMES)
def test_check_bias_accepts_the_host_encoder(name):
    records, recs, ads, addends, total, wire = _encoded(name)
    assert _both(recs, ads, len(records), wire, len(wire), total) == (0, 0), _lib.load().tk_last_error()


def test_check_bias_refuses_what_the_decoder_refuses():
    records, recs, ads, addends, total, wire = _encoded()
    n = len(records)
    seg_n = [(i, min(wc.SEG, len(r) - s)) for i, r in enumerate(records) for s in range(0, len(r), wc.SEG)]
    table = wc._a(4 * len(seg_n), 64)
    # the last segment is a bias record's: headers alone, which end inside the last 64 bytes
    nb = (seg_n[-1][1] + wc.BLOCK - 1) // wc.BLOCK
    start = int(wire[4 * (len(seg_n) - 1):4 * len(seg_n)].view(np.uint32)[0])
    end = table + 64 * start + wc._a(4 * nb, 16) + wc._a(nb, 16)
    assert end <= len(wire) < end + 64
    assert _both(recs, ads, n, wire, end, total) == (0, 0)
    assert _both(recs, ads, n, wire, end - 1, total) == (INVALID_ARG, INVALID_ARG)      # one byte short
    bad = wire.copy()   # a width of 5, in a segment of the bias-coded record 1
    seg = next(k for k, (i, _) in enumerate(seg_n) if i == 1)
    nb1 = (seg_n[seg][1] + wc.BLOCK - 1) // wc.BLOCK
    at = table + 64 * int(wire[4 * seg:4 * seg + 4].view(np.uint32)[0]) + wc._a(4 * nb1, 16)
    bad[at] = 5
    assert _both(recs, ads, n, bad, len(bad), total) == (INVALID_ARG, INVALID_ARG)
    bad = wire.copy()   # a start beyond the payload
    bad[4 * seg:4 * seg + 4].view(np.uint32)[0] = (len(wire) - table) // 64 + 1
    assert _both(recs, ads, n, bad, len(bad), total) == (INVALID_ARG, INVALID_ARG)
    # no addend value is read: pointers to nothing pass the check
    for i in range(n):
        if addends[i] is not None:
            ads[i].addend = 4096
    exact = wire.copy()
    assert _lib.load().tk_wire_check_bias(recs, ads, n, wc.ptr(exact), len(exact)) == 0


# ---------------------------------------------------------------- files built in Python (no library)
def _plan_entry(name, shape, coding, diff, extra=b""):
    nm = name.encode()
    return (struct.pack("<H", len(nm)) + nm + struct.pack("<5B", 0, 32, len(shape), coding, diff) +
            struct.pack(f"<{len(shape)}q", *shape) + extra)


def _file(version, entries, addend_size=None, wire=b"\0" * 64, addends=b"", raw=b""):
    """A packed file around `entries` (plan bytes); nothing but parse_packed's own rules is meant to
    hold: the wire is 64 zero bytes."""
    plan = b"".join(entries)
    if version == 3:
        head = struct.pack("<IIQQQQ", tf.PACK_MAGIC, len(entries), len(plan), len(wire), len(raw), addend_size)
    else:
        head = struct.pack("<IIQQQ", tf.PACK_MAGIC, len(entries), len(plan), len(wire), len(raw))
    head += plan
    section = head + b"\0" * (-len(head) % 8) + addends + wire + raw
    text = json.dumps({"n_samples": 2}).encode()
    po = ro = 4096
    return (struct.pack("<7Q", tf.TRACE_MAGIC, version, len(text), po, 0, ro, len(section)) + text +
            b"\0" * (4096 - 56 - len(text)) + section)


def _good(shape=(2, 3, 5), axis=1, addend_off=0, diff=1, coding=3, prev_shape=None, prev_coding=0, addend_size=16,
          addends=None, bits=None, extra=None):
    prev = _plan_entry("a", shape if prev_shape is None else prev_shape, prev_coding, 0)
    rec = _plan_entry("b", shape, coding, diff, struct.pack("<BQ", axis, addend_off) if extra is None else extra)
    if prev_coding == 1:   # an int8 predecessor
        prev = prev.replace(struct.pack("<5B", 0, 32, len(shape), 1, 0), struct.pack("<5B", 0, 8, len(shape), 1, 0))
    if bits is not None:
        rec = rec.replace(struct.pack("<5B", 0, 32, len(shape), coding, diff), struct.pack("<5B", 0, bits, len(shape), coding, diff))
    return _file(3, [prev, rec], addend_size, addends=b"\0" * addend_size if addends is None else addends)


def test_reader_refuses_each_broken_field():
    pf = tf.parse_packed(_good())
    assert pf.version == 3 and pf.entries[1].coding == tf.BIAS and (pf.entries[1].channels, pf.entries[1].plane) == (3, 5)
    assert pf.addend_size == 16 and pf.wire_off == pf.addend_off + 16
    broken = {
        "no diff": _good(diff=0),
        "not int32": _good(bits=8),
        "2^31 elements": _good(shape=(2, 1 << 30, 1)),
        "predecessor not int32": _good(prev_coding=1),
        "predecessor raw": _file(3, [_plan_entry("a", (2, 3, 5), tf.RAW, 0, struct.pack("<QQ", 0, 120)),
                                     _plan_entry("b", (2, 3, 5), 3, 1, struct.pack("<BQ", 1, 0))], 16, addends=b"\0" * 16,
                                 raw=b"\0" * 120),
        "predecessor of another count": _good(prev_shape=(2, 3, 4)),
        "no predecessor": _file(3, [_plan_entry("b", (2, 3, 5), 3, 1, struct.pack("<BQ", 1, 0))], 16, addends=b"\0" * 16),
        "axis >= ndim": _good(axis=3),
        "addends outside the part": _good(addend_off=8),
        "addend offset no multiple of 4": _good(addend_off=2),
        "addends part larger than the section": _good(addend_size=24, addends=b"\0" * 16),
        "addends part no multiple of 8": _good(addend_size=12, addends=b"\0" * 12),
        "plan entry cut short": _good(extra=b"\1"),
    }
    for what, data in broken.items():
        with pytest.raises(ValueError):
            tf.parse_packed(data)
            pytest.fail(what)
        with pytest.raises(ValueError):
            tf.check_trace(np.frombuffer(data, np.uint8), [("a", (2, 3, 5), "int32"), ("b", (2, 3, 5), "int32")])
    # a bias axis of no channels: the record has no elements, which no coded entry may
    with pytest.raises(ValueError):
        tf.parse_packed(_good(shape=(2, 0, 5)))
    # coding 3 is a version-3 coding: the same entry in a version-2 section is refused
    with pytest.raises(ValueError):
        tf.parse_packed(_file(2, [_plan_entry("a", (2, 3, 5), 0, 0), _plan_entry("b", (2, 3, 5), 3, 1)]))


def test_version_2_layout_is_untouched():
    assert tf.PACKED_VERSION == 2 and tf.PACKED_VERSIONS == (2, 3)
    items = [("a", (2, 3, 5), "int32"), ("b", (2, 3, 5), "int32"), ("f", (4,), "float32")]
    entries = tf.packed_entries(items)
    assert [(e.coding, e.diff) for e in entries] == [(0, 0), (0, 1), (tf.RAW, 0)]
    plan = (_plan_entry("a", (2, 3, 5), 0, 0) + _plan_entry("b", (2, 3, 5), 0, 1) +
            struct.pack("<H", 1) + b"f" + struct.pack("<5B", 2, 32, 1, tf.RAW, 0) + struct.pack("<q", 4) +
            struct.pack("<QQ", 0, 16))
    head = struct.pack("<IIQQQ", tf.PACK_MAGIC, 3, len(plan), 640, 16) + plan
    assert tf.packed_section_head(entries, 640) == head + b"\0" * (-len(head) % 8)
    pf = tf.parse_packed(_file(2, [_plan_entry("a", (2, 3, 5), 0, 0), _plan_entry("b", (2, 3, 5), 0, 1)]))
    assert (pf.version, pf.addend_size) == (2, 0)


def test_pack_trace_without_bias_is_version_2():
    records, diffs, addends, _ = wb.cases(np.random.default_rng(7))["grid_49_24_2"]
    v1 = _v1(records, addends)
    v2 = tf.pack_trace(v1)
    assert v2 == tf.pack_trace(v1, bias=False)
    assert struct.unpack_from("<Q", v2, 8)[0] == 2
    # the file restated: the version-1 head, the version-2 section header and plan, tk_wire_encode_host's bytes
    lib = _lib.load()
    arrays = tf.read_trace(v1).records
    base = np.frombuffer(v1, np.uint8)
    offs = [v.ctypes.data - base.ctypes.data for v in arrays.values()]
    recs = wc.wire_records([v.reshape(-1) for v in arrays.values()], diffs, offs)
    bound = lib.tk_wire_bound(recs, 2)
    wire = np.zeros(bound, np.uint8)
    used = lib.tk_wire_encode_host(recs, 2, wc.ptr(base), len(v1), wc.ptr(wire), bound)
    shape = tuple(arrays["r0"].shape)
    plan = _plan_entry("r0", shape, 0, 0) + _plan_entry("r1", shape, 0, 1)
    head = struct.pack("<IIQQQ", tf.PACK_MAGIC, 2, len(plan), used, 0) + plan
    section = head + b"\0" * (-len(head) % 8) + wire[:used].tobytes()
    ro = struct.unpack_from("<Q", v1, 40)[0]
    assert v2 == v1[:8] + struct.pack("<Q", 2) + v1[16:48] + struct.pack("<Q", len(section)) + v1[56:ro] + section
    assert tf.unpack_trace(v2) == v1 and tf.parse_packed(v2).version == 2
