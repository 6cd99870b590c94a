"""Packed (version 2) trace files on the host (tachikoma_amd/trace_format.py): pack_trace /
unpack_trace round trips of a synthetic trace that holds every coding the plan can choose, the
stored plan against the planning rule (and a reader that follows the file, not the rule), refusal
of truncated and corrupted files, and the trace job's "packed" journal flag with a stub tracer.
The device packer is covered by tests/test_gpu_trace_packed.py."""
import concurrent.futures
import json
import struct

import numpy as np
import pytest

from tachikoma_amd import _lib, trace_job
from tachikoma_amd import trace_format as tf
from tests import wire_cases as wc
from tests import wire_cases8 as w8

BIG = 2 * 16384 + 300


def _records():
    rng = np.random.default_rng(2)
    chain, _ = wc.contents(3 * 256 + 17, rng)["diff_chain"]                 # int32, same shape: a diff chain
    prev8, clip8 = w8.contents(BIG, 1, rng)["both_bounds"][0]               # int8 and a true clip of it
    noise8 = w8.contents(BIG, 1, rng)["random_plain"][0][0]                 # follows clip8, is no clip of it
    prevu, clipu = w8.contents(700, 2, rng)["u8_above_127"][0]
    return {
        "data": rng.standard_normal((2, 3, 5)).astype(np.float32),          # the graph input, float32: raw
        "%0": chain[0].reshape(1, -1), "%1": chain[1].reshape(1, -1), "%2": chain[2].reshape(1, -1),
        "%3": prev8, "%4": clip8, "%5": noise8,
        "%6": prevu.reshape(2, 350), "%7": clipu.reshape(2, 350),
        "%8": np.arange(-9, 9, dtype=np.int16),
        "%9": np.arange(5, dtype=np.int64) << 40,
        "%10": np.array([-7], np.int32),                                    # one element
        "%11": rng.integers(-2 ** 31, 2 ** 31, BIG, dtype=np.int64).astype(np.int32),
        "%12": rng.standard_normal(33).astype(np.float32),
    }


@pytest.fixture(scope="module")
def synthetic():
    recs = _records()
    meta = {"format": "tachikoma-trace", "sample_offset": 4, "n_samples": 2, "inputs": ["data"]}
    params = {"w": np.arange(24, dtype=np.int8).reshape(2, 3, 4), "b": np.arange(3, dtype=np.int32)}
    v1 = tf.trace_bytes(meta, params, recs)
    return recs, v1, tf.pack_trace(v1)


def _items(recs):
    return [(k, v.shape, str(v.dtype)) for k, v in recs.items()]


def test_round_trip_is_byte_exact(synthetic, tmp_path):
    recs, v1, v2 = synthetic
    assert struct.unpack_from("<2Q", v2, 0) == (tf.TRACE_MAGIC, tf.PACKED_VERSION)
    assert tf.unpack_trace(v2) == v1
    a, b = tf.read_trace(v1), tf.read_trace(v2)
    assert a.meta == b.meta and list(a.records) == list(b.records) == list(recs)
    for k, v in recs.items():
        assert b.records[k].dtype == v.dtype and np.array_equal(b.records[k], v), k
    assert list(a.params) == list(b.params) and all(np.array_equal(a.params[k], b.params[k]) for k in a.params)
    assert tf.trace_file_digest(v2) == tf.trace_file_digest(v1) == tf.records_digest(recs)
    # from files, as the CLI does it
    p1, p2, p3 = (str(tmp_path / n) for n in ("a.tkt", "a.packed.tkt", "b.tkt"))
    open(p1, "wb").write(v1)
    assert tf.main(["pack", p1, p2]) == 0 and open(p2, "rb").read() == v2
    assert tf.main(["unpack", p2, p3]) == 0 and open(p3, "rb").read() == v1
    assert tf.main(["info", p2]) == 0
    assert tf.trace_file_digest(p2) == tf.records_digest(recs)


def test_size_is_within_the_formats_worst_case(synthetic):
    """len(packed) <= len(v1) + tk_wire_bound - bytes of the coded records: a condition of the
    format (every block raw), not a measurement."""
    recs, v1, v2 = synthetic
    entries = tf.packed_entries(_items(recs))
    arr, n = tf._wire_records(entries, [0] * len(entries))
    bound = _lib.load().tk_wire_bound(arr, n)
    coded = sum(e.nbytes for e in entries if e.coding != tf.RAW)
    assert bound > 0 and coded > 0
    assert len(v2) <= len(v1) + bound - coded
    # every record a single raw-width int32 block: the worst case itself still holds
    rng = np.random.default_rng(5)
    worst = {f"%{i}": rng.integers(-2 ** 31, 2 ** 31, 5, dtype=np.int64).astype(np.int32) for i in range(3)}
    w1 = tf.trace_bytes({}, {}, worst)
    e = tf.packed_entries(_items(worst))
    arr, n = tf._wire_records(e, [0] * 3)
    assert len(tf.pack_trace(w1)) <= len(w1) + _lib.load().tk_wire_bound(arr, n) - 60
    assert tf.unpack_trace(tf.pack_trace(w1)) == w1


def test_stored_plan_is_the_planning_rule(synthetic):
    recs, _, v2 = synthetic
    plan = tf.plan_records(_items(recs))
    pf = tf.parse_packed(v2)
    assert [(e.coding, e.diff) for e in pf.entries] == plan
    assert [(e.name, e.shape, e.dtype) for e in pf.entries] == [(k, v.shape, str(v.dtype)) for k, v in recs.items()]
    R = tf.RAW
    assert dict(zip(recs, plan)) == {
        "data": (R, 0), "%0": (0, 0), "%1": (0, 1), "%2": (0, 1), "%3": (1, 0), "%4": (1, 1), "%5": (1, 1),
        "%6": (2, 0), "%7": (2, 1), "%8": (R, 0), "%9": (R, 0), "%10": (0, 0), "%11": (0, 0), "%12": (R, 0)}
    # a record of the same dtype but another shape starts a new chain; one after a raw record too
    assert tf.plan_records([("a", (4, 4), "int32"), ("b", (16,), "int32"), ("c", (2,), "float32"),
                            ("d", (16,), "int32"), ("e", (0,), "int8")]) == [(0, 0), (0, 0), (R, 0), (0, 0), (R, 0)]
    # the clip is coded as a clamp (its blocks cost no payload), the record that is no clip escapes
    info = tf.packed_info(v2)
    assert info["wire_bytes"] == pf.wire_size and info["records"] == len(recs)
    raw = sum(v.nbytes for k, v in recs.items() if plan[list(recs).index(k)][0] == R)
    assert pf.raw_size == raw


def _repack_with_plan(v1, recs, plan):
    """The packed file of v1 coded by `plan` instead of the rule's plan (host encoder)."""
    lib = _lib.load()
    tr_off = [v.ctypes.data for v in tf.read_trace(v1).records.values()]
    base = np.frombuffer(v1, np.uint8).ctypes.data
    entries = tf.packed_entries(_items(recs), plan)
    arr, n = tf._wire_records(entries, [o - base for o in tr_off])
    bound = lib.tk_wire_bound(arr, n)
    wire = np.zeros(bound, np.uint8)
    used = lib.tk_wire_encode_host(arr, n, wc.ptr(np.frombuffer(v1, np.uint8)), len(v1), wc.ptr(wire), bound)
    assert used > 0, lib.tk_last_error()
    ro = struct.unpack_from("<7Q", v1, 0)[5]
    section = tf.packed_section_head(entries, used) + wire[:used].tobytes() + \
        b"".join(v.tobytes() for e, v in zip(entries, recs.values()) if e.coding == tf.RAW)
    return struct.pack("<2Q", tf.TRACE_MAGIC, tf.PACKED_VERSION) + v1[16:48] + struct.pack("<Q", len(section)) + \
        v1[56:ro] + section


def test_reader_follows_the_stored_plan(synthetic):
    """Legal variants of the plan, packed accordingly, unpack to the same file: a diff flag cleared,
    a clamp prediction dropped, a codable record stored raw.  (The rule's own plan through the same
    helper gives pack_trace's bytes.)"""
    recs, v1, v2 = synthetic
    names = list(recs)
    plan = tf.plan_records(_items(recs))
    assert _repack_with_plan(v1, recs, plan) == v2
    for name, coding in (("%1", (0, 0)), ("%4", (1, 0)), ("%7", (2, 0)), ("%11", (tf.RAW, 0)), ("%3", (tf.RAW, 0))):
        alt = list(plan)
        i = names.index(name)
        alt[i] = coding
        if coding[0] == tf.RAW and i + 1 < len(alt) and alt[i + 1][1]:
            alt[i + 1] = (alt[i + 1][0], 0)      # its successor has no coded predecessor any more
        other = _repack_with_plan(v1, recs, alt)
        assert other != v2
        assert [(e.coding, e.diff) for e in tf.parse_packed(other).entries] == alt
        assert tf.unpack_trace(other) == v1, name
        assert tf.trace_file_digest(other) == tf.trace_file_digest(v1)


def test_truncated_and_corrupted_files_are_refused(synthetic):
    recs, v1, v2 = synthetic
    pf = tf.parse_packed(v2)
    _, _, jl, po, ps, ro, rs = struct.unpack_from("<7Q", v2, 0)
    plan_end = ro + 32 + struct.unpack_from("<IIQQQ", v2, ro)[2]
    boundaries = [0, 8, 56, 56 + jl, po, po + ps, ro, ro + 32, plan_end, pf.wire_off, pf.raw_off, len(v2) - 1]
    inside_wire = [pf.wire_off + 1, pf.wire_off + 64, pf.wire_off + pf.wire_size // 2, pf.raw_off - 1]
    for cut in boundaries + inside_wire:
        assert cut < len(v2)
        for f in (tf.unpack_trace, tf.read_trace, tf.trace_file_digest):
            with pytest.raises(ValueError):
                f(v2[:cut])
    # the header patched to the shorter length as well (the sections then do not add up)
    for cut in inside_wire:
        short = bytearray(v2[:cut])
        struct.pack_into("<Q", short, 48, cut - ro)
        with pytest.raises(ValueError):
            tf.unpack_trace(bytes(short))
    # a wire_size that claims less than the segments need: the decoder refuses the last segments
    lie = bytearray(v2)
    cutw = pf.wire_size - 4096
    del lie[pf.wire_off + cutw:pf.raw_off]
    struct.pack_into("<Q", lie, ro + 16, cutw)
    struct.pack_into("<Q", lie, 48, rs - 4096)
    with pytest.raises(ValueError):
        tf.unpack_trace(bytes(lie))
    # a table entry pointing past the end of the wire buffer
    for seg, start in ((0, 0xFFFFFFFF), (3, pf.wire_size // 64), (5, pf.wire_size // 64 - 1)):
        bad = bytearray(v2)
        struct.pack_into("<I", bad, pf.wire_off + 4 * seg, start)
        with pytest.raises(ValueError):
            tf.unpack_trace(bytes(bad))
    # a width no segment of that kind may state; a plan that does not fit the record list
    bad = bytearray(v2)
    nb = (3 * 256 + 17 + 255) // 256
    table = (4 * sum((v.size + 16383) // 16384 for v, e in zip(recs.values(), pf.entries) if e.coding != tf.RAW)
             + 63) // 64 * 64
    bad[pf.wire_off + table + 16] = 9      # first width byte of segment 0 (4 bases padded to 16 B)
    assert nb == 4
    with pytest.raises(ValueError):
        tf.unpack_trace(bytes(bad))
    at = v2.index(b"\x02\x00%1", ro) + 4   # entry "%1": code, bits, ndim, coding, diff
    assert v2[at:at + 5] == bytes([0, 32, 2, 0, 1])
    for field, value in ((3, 1), (3, 7), (4, 2), (1, 8), (2, 3)):
        bad = bytearray(v2)
        bad[at + field] = value
        with pytest.raises(ValueError):
            tf.unpack_trace(bytes(bad))
    first = bytearray(v2)                  # diff on a record whose predecessor is raw
    at0 = v2.index(b"\x02\x00%0", ro) + 4
    first[at0 + 4] = 1
    with pytest.raises(ValueError):
        tf.unpack_trace(bytes(first))
    with pytest.raises(ValueError):
        tf.pack_trace(v2)                  # wants a version-1 file
    with pytest.raises(ValueError):
        tf.unpack_trace(v1)


class StubTracer:
    """Writes the chunk files from host arrays: packed or not, as a device tracer would."""

    def __init__(self, packed):
        self.packed = packed
        self.calls = []

    def __call__(self, offset, n, path):
        self.calls.append(offset)
        a = (np.arange(n * 300, dtype=np.int32).reshape(n, 300) + offset) * 3
        recs = {"data": np.full((n, 4), offset, np.int8), "%0": a, "%1": a + 5, "%2": np.clip(a, 0, 100).astype(np.int8)}
        v1 = tf.trace_bytes({"sample_offset": offset, "n_samples": n}, {}, recs)
        with open(path, "wb") as f:
            f.write(tf.pack_trace(v1) if self.packed else v1)
        fut = concurrent.futures.Future()
        fut.set_result(tf.records_digest(recs))
        return fut


def _journal(d):
    return [json.loads(ln) for ln in open(trace_job.journal_file(d, 0)).read().strip().split("\n")]


def test_journal_records_the_packed_flag(tmp_path):
    d, ref = str(tmp_path / "packed"), str(tmp_path / "plain")
    t = StubTracer(True)
    entries = trace_job.run(t, 7, 2, d)                    # the flag is the tracer's own
    plain = trace_job.run(StubTracer(False), 7, 2, ref)
    assert t.calls == [0, 2, 4, 6]
    assert [e["packed"] for e in _journal(d)] == [True] * 4
    assert [e["packed"] for e in _journal(ref)] == [False] * 4
    # same names, same digests (of the records, not of the file), fewer bytes; each unpacks to the plain file
    assert [(e.file, e.digest) for e in entries] == [(e.file, e.digest) for e in plain]
    for e, j, jp in zip(entries, _journal(d), _journal(ref)):
        packed = open(f"{d}/{e.file}", "rb").read()
        assert tf.unpack_trace(packed) == open(f"{ref}/{e.file}", "rb").read()
        assert j["bytes"] == len(packed) < jp["bytes"]
    # nothing to do on a resume of the same kind, --verify included (it digests the packed files)
    for verify in (False, True):
        again = StubTracer(True)
        trace_job.run(again, 7, 2, d, verify=verify)
        assert again.calls == []
    # a corrupted packed chunk fails verification and is traced again
    c1 = trace_job.chunk_file(d, 0, 1)
    raw = bytearray(open(c1, "rb").read())
    raw[tf.parse_packed(bytes(raw)).wire_off + 64 + 64 + 100] ^= 0x55    # a plane byte of %0 (table, data's segment)
    open(c1, "wb").write(bytes(raw))
    again = StubTracer(True)
    trace_job.run(again, 7, 2, d, verify=True)
    assert again.calls == [2]


def test_flag_mismatch_forces_a_retrace(tmp_path):
    d = str(tmp_path)
    trace_job.run(StubTracer(False), 6, 2, d)
    # entries written before the flag existed count as unpacked
    lines = [{k: v for k, v in e.items() if k != "packed"} for e in _journal(d)]
    open(trace_job.journal_file(d, 0), "w").write("".join(json.dumps(e) + "\n" for e in lines))
    t = StubTracer(False)
    trace_job.run(t, 6, 2, d)
    assert t.calls == [] and "packed" not in _journal(d)[0]
    # one chunk's entry already says packed (a job of the other kind got that far)
    trace_job.Journal(trace_job.journal_file(d, 0)).append(dict(_journal(d)[1], packed=True))
    t = StubTracer(False)
    trace_job.run(t, 6, 2, d)
    assert t.calls == [2]
    # a packed job over an unpacked directory traces every chunk again, and the files become packed
    t = StubTracer(True)
    entries = trace_job.run(t, 6, 2, d, packed=True)
    assert t.calls == [0, 2, 4]
    for e in entries:
        assert struct.unpack_from("<2Q", open(f"{d}/{e.file}", "rb").read(), 0)[1] == tf.PACKED_VERSION
    done = trace_job.Journal(trace_job.journal_file(d, 0)).entries()
    assert all(done[i]["packed"] is True for i in range(3))
