"""tk_wire_check, the host gate of the device wire decoder: it accepts what the host encoder writes,
refuses what tk_wire_decode refuses (and nothing else) without reading a payload byte, and
trace_format.check_trace, the host half of GraphModule.verify_trace, refuses truncated files, bad
plans and traces of another graph.  No device is involved."""
import struct

import numpy as np
import pytest

from tachikoma_amd import _lib
from tachikoma_amd import trace_format as tf
from tests import wire_cases as wc
from tests import wire_cases8 as w8

OK, INVALID = 0, -1


def _encode(records, diffs):
    lib = _lib.load()
    offs, total = w8.layout(records)
    recs = w8.wire_records(records, diffs, offs)
    src = w8.image_of(records, offs, total)
    bound = lib.tk_wire_bound(recs, len(records))
    assert bound > 0, lib.tk_last_error()
    wire = np.zeros(bound, np.uint8)
    used = lib.tk_wire_encode_host(recs, len(records), w8.ptr(src), total, w8.ptr(wire), bound)
    assert used > 0, lib.tk_last_error()
    return recs, offs, total, src, wire[:used].copy()


def _check(recs, n, wire, nbytes=None):
    # a copy of exactly the stated size: nothing behind it to fall back on
    nbytes = len(wire) if nbytes is None else nbytes
    exact = wire[:max(nbytes, 0)].copy() if nbytes > 0 else np.zeros(1, np.uint8)
    return _lib.load().tk_wire_check(recs, n, w8.ptr(exact), nbytes)


def _decode(recs, n, wire, total):
    out = np.zeros(total, np.uint8)
    return _lib.load().tk_wire_decode(recs, n, w8.ptr(wire), len(wire), w8.ptr(out), total, 1)


@pytest.mark.parametrize("n", sorted(set(wc.SIZES) | set(w8.SIZES)))
def test_check_accepts_the_host_encoder(n):
    rng = np.random.default_rng(n)
    cases = []
    if n in wc.SIZES:
        cases += sorted(wc.contents(n, rng).items())
    if n in w8.SIZES:
        for kind in sorted(w8.KINDS):
            cases += sorted(w8.contents(n, kind, rng).items())
    for name, (records, diffs) in cases:
        recs, offs, total, src, wire = _encode(records, diffs)
        assert _check(recs, len(records), wire) == OK, (name, _lib.load().tk_last_error())


def _mixed(n=2 * 16384 + 300, seed=5):
    """An int32 chain, an int8 clamp pair and a plain uint8 record in one buffer."""
    rng = np.random.default_rng(seed)
    chain, cdiff = wc.contents(n, rng)["diff_chain"]
    pair, pdiff = w8.contents(n, 1, rng)["both_bounds"]
    plain, qdiff = w8.contents(n, 2, rng)["random_plain"]
    return chain + pair + plain, cdiff + pdiff + qdiff


def _header_at(wire, n_seg, seg, n):
    """(offset of segment `seg`'s header in the buffer, its base bytes, its blocks)."""
    table = wc._a(4 * n_seg, 64)
    start = int(wire[4 * seg:4 * seg + 4].view(np.uint32)[0])
    nb = (n + wc.BLOCK - 1) // wc.BLOCK
    return table + 64 * start, wc._a(4 * nb, 16), nb


def test_check_refusals():
    lib = _lib.load()
    records, diffs = _mixed()
    nrec = len(records)
    recs, offs, total, src, wire = _encode(records, diffs)
    seg_n = [(i, min(wc.SEG, len(r) - s)) for i, r in enumerate(records) for s in range(0, len(r), wc.SEG)]
    n_seg = len(seg_n)
    table = wc._a(4 * n_seg, 64)
    assert _check(recs, nrec, wire) == OK
    # wire_bytes below the table
    assert _check(recs, nrec, wire, table - 1) == INVALID and b"table" in lib.tk_last_error()
    assert _check(recs, nrec, wire, 0) == INVALID
    # cut one byte short of the last segment's end (the host encoder lays segments in order, and the
    # last one, a raw uint8 plane, ends within the last 64 bytes)
    last_seg, last_n = n_seg - 1, seg_n[-1][1]
    at, base_bytes, nb = _header_at(wire, n_seg, last_seg, last_n)
    end = at + base_bytes + wc._a(nb, 16) + last_n   # every block of random_plain is raw
    assert end <= len(wire) < end + 64
    assert _check(recs, nrec, wire, end) == OK
    assert _check(recs, nrec, wire, end - 1) == INVALID
    # a table entry past the end
    bad = wire.copy()
    bad[4:8].view(np.uint32)[0] = 0xFFFFFFFF
    assert _check(recs, nrec, bad) == INVALID and _decode(recs, nrec, bad, total) == INVALID
    bad = wire.copy()
    bad[0:4].view(np.uint32)[0] = (len(wire) - table) // 64 + 1
    assert _check(recs, nrec, bad) == INVALID
    # width 5 in an int32 segment (record 0), width 2 in a 1-byte segment (record 3, int8)
    for rec, width in ((0, 5), (3, 2)):
        seg = next(k for k, (i, _) in enumerate(seg_n) if i == rec)
        at, base_bytes, nb = _header_at(wire, n_seg, seg, seg_n[seg][1])
        bad = wire.copy()
        bad[at + base_bytes + nb - 1] = width
        assert _check(recs, nrec, bad) == INVALID, (rec, width)
        assert _decode(recs, nrec, bad, total) == INVALID
    # the records' rules are host_plan's: a diff record after one of another size, or of another kind
    recs[1].n_elems += 1
    assert _check(recs, nrec, wire) == INVALID
    recs[1].n_elems -= 1
    recs[4].kind = 2
    assert _check(recs, nrec, wire) == INVALID
    assert lib.tk_wire_check(recs, 0, w8.ptr(wire), len(wire)) == INVALID
    assert lib.tk_wire_check(None, nrec, w8.ptr(wire), len(wire)) == INVALID


def test_check_agrees_with_the_decoder_on_corrupted_headers():
    """500 seeded single-byte corruptions of table and header bytes (never payload) of a mixed-kind
    buffer: the gate says OK exactly when the decoder does.  Positions are drawn half from the table
    entries' low two bytes and the width bytes (which mostly break the buffer: a start moved by up to
    4 MiB leaves it, a width above the kind's is refused, a larger width lengthens a segment past the
    end only sometimes) and half from the base bytes (which never do), so that both outcomes occur
    often; the counts are asserted."""
    records, diffs = _mixed(n=16384 + 700, seed=9)
    nrec = len(records)
    recs, offs, total, src, wire = _encode(records, diffs)
    seg_n = [(i, min(wc.SEG, len(r) - s)) for i, r in enumerate(records) for s in range(0, len(r), wc.SEG)]
    n_seg = len(seg_n)
    structural, bases = [], []
    for seg, (rec, n) in enumerate(seg_n):
        structural += [4 * seg, 4 * seg + 1, 4 * seg + 2, 4 * seg + 3]
        at, base_bytes, nb = _header_at(wire, n_seg, seg, n)
        structural += list(range(at + base_bytes, at + base_bytes + nb))
        bases += list(range(at, at + 4 * nb))
    rng = np.random.default_rng(2024)
    seen = {OK: 0, INVALID: 0}
    for trial in range(500):
        pool = structural if trial % 2 == 0 else bases
        pos = int(pool[rng.integers(len(pool))])
        bad = wire.copy()
        bad[pos] ^= int(rng.integers(1, 256))
        got, want = _check(recs, nrec, bad), _decode(recs, nrec, bad, total)
        assert got == want, (trial, pos, got, want)
        seen[want] += 1
    assert seen[OK] >= 50 and seen[INVALID] >= 50, seen


# ---------------------------------------------------------------- check_trace (verify_trace's host half)
def _trace_bytes(batch=2, seed=0, names=("data", "%0", "%1", "%2", "%3")):
    rng = np.random.default_rng(seed)
    acc = rng.integers(-50000, 50000, (batch, 4, 5, 5), dtype=np.int64).astype(np.int32)
    q = rng.integers(-128, 128, (batch, 4, 5, 5), dtype=np.int64).astype(np.int8)
    arrays = [rng.integers(-128, 128, (batch, 3, 5, 5), dtype=np.int64).astype(np.int8), acc, acc + 7, q,
              np.clip(q, 0, 127).astype(np.int8)]
    records = dict(zip(names, arrays))
    params = {"w": rng.integers(-9, 9, (4, 3, 1, 1), dtype=np.int64).astype(np.int8),
              "scale": rng.random(4).astype(np.float32)}
    meta = {"format": "tachikoma-trace", "n_samples": batch}
    return tf.trace_bytes(meta, params, records), records, params


def _items(arrays):
    return [(k, v.shape, str(v.dtype)) for k, v in arrays.items()]


def test_check_trace_accepts_both_versions():
    plain, records, params = _trace_bytes()
    packed = tf.pack_trace(plain)
    for blob in (plain, packed):
        ct = tf.check_trace(blob, _items(records), _items(params))
        assert [e.name for e in ct.entries] == list(records) and ct.size == len(blob)
        assert ct.meta["n_samples"] == 2
        assert sorted(p[0] for p in ct.params) == sorted(params)
        for name, shape, dtype, off in ct.params:
            n = params[name].nbytes
            assert bytes(blob[off:off + n]) == params[name].tobytes()
    ct = tf.check_trace(packed, _items(records))
    assert ct.packed and ct.wire_size > 0 and [e.coding for e in ct.entries] == [1, 0, 0, 1, 1]
    assert [e.diff for e in ct.entries] == [0, 0, 1, 0, 1]
    ct = tf.check_trace(plain, _items(records))
    assert not ct.packed and ct.wire_size == 0
    for e in ct.entries:   # version 1: every record raw, at its place in the blob
        at = ct.records_off + e.raw_off
        assert bytes(plain[at:at + e.raw_size]) == records[e.name].tobytes()


def test_check_trace_refuses_truncated_files():
    plain, records, params = _trace_bytes()
    packed = tf.pack_trace(plain)
    for blob in (plain, packed):
        for cut in (1, 100, len(blob) - 60, len(blob) - 10):
            with pytest.raises(ValueError):
                tf.check_trace(blob[:len(blob) - cut], _items(records), _items(params))
    with pytest.raises(ValueError):
        tf.check_trace(b"", _items(records))


def test_check_trace_refuses_a_bad_plan_and_a_bad_wire():
    plain, records, params = _trace_bytes()
    packed = bytearray(tf.pack_trace(plain))
    pf = tf.parse_packed(bytes(packed))
    # the plan: record 2 (differenced int32) claims to be a uint8 record
    ro = struct.unpack_from("<7Q", packed, 0)[5]
    plan_at = ro + tf._SECTION.size
    blob = bytes(packed)
    at = blob.index(b"%1", plan_at) + 2 + 3      # name, then code, bits, ndim -> coding
    bad = bytearray(packed)
    bad[at] = 2
    with pytest.raises(ValueError):
        tf.check_trace(bytes(bad), _items(records))
    # the wire: a table entry far outside (tk_wire_check), and a width the kind does not have
    bad = bytearray(packed)
    bad[pf.wire_off:pf.wire_off + 4] = b"\xff\xff\xff\xff"
    with pytest.raises(ValueError, match="tk_wire_check"):
        tf.check_trace(bytes(bad), _items(records))
    assert tf.check_trace(bytes(packed), _items(records)).wire_size == pf.wire_size
    # the same refusal on a numpy view, which is what the verifier's pinned staging is
    with pytest.raises(ValueError, match="tk_wire_check"):
        tf.check_trace(np.frombuffer(bytes(bad), np.uint8), _items(records))


def test_check_trace_refuses_another_graph():
    plain, records, params = _trace_bytes()
    packed = tf.pack_trace(plain)
    other, other_records, _ = _trace_bytes(names=("data", "%0", "%1", "%2", "%9"))
    bigger, bigger_records, _ = _trace_bytes(batch=3)
    for blob in (plain, packed):
        for want in (_items(other_records), _items(bigger_records), _items(records)[:-1],
                     list(reversed(_items(records)))):
            with pytest.raises(ValueError, match="another graph"):
                tf.check_trace(blob, want, _items(params))
        with pytest.raises(ValueError, match="another graph"):
            tf.check_trace(blob, _items(records), _items(params)[:1])
        wrong_dtype = [(k, s, "uint8" if k == "%3" else d) for k, s, d in _items(records)]
        with pytest.raises(ValueError, match="another graph"):
            tf.check_trace(blob, wrong_dtype)
