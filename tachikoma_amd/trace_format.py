"""The tachikoma trace binary: writer (through the C ABI) and a numpy reader.

Container (``include/tachikoma.h``, "trace format")::

    tk_trace_header  {"TKTRACE\\0", version, json_len, params_off, params_size,
                      records_off, records_size}       (7 × u64, little-endian)
    json             op table + run metadata (utf-8, space padded)
    pad to 4096
    params blob      NDArray-list (src/runtime/file_utils.cc:210-236) of the weights
    pad to 4096
    records blob     NDArray-list of every traced tensor: graph inputs, then every
                     op output in topological order, keyed by MRT symbol name (%N)

Each record is the whole batch shard of that op output ([B_shard, ...]), i.e.
exactly what ``mrt.Trace.calibrate`` returns per symbol
(python/tvm/mrt/trace.py:65-117); ``sample_offset`` in the json places the shard
in the global batch.  The NDArray-list encoding makes the params/records
sections loadable by the reference's own ``LoadParams`` / CRT reader.
"""
from __future__ import annotations

import ctypes
import json
import mmap
import os
import struct
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

TRACE_MAGIC = 0x0045434152544B54
TRACE_VERSION = 1
TRACE_ALIGN = 4096
LIST_MAGIC = 0xF7E58D4F05049CB7
ARRAY_MAGIC = 0xDD5E40F096B4A13F
JSON_SLACK = 256  # header json is space-padded so per-shard fields can be rewritten in place


def _metas(items: Sequence[Tuple[str, Sequence[int], str]]):
    """Build a ctypes tk_array_meta array (+ keepalive list)."""
    keep = []
    arr = (_lib.tk_array_meta * max(1, len(items)))()
    for i, (name, shape, dtype) in enumerate(items):
        nm = name.encode()
        sh = (ctypes.c_int64 * max(1, len(shape)))(*[int(s) for s in shape])
        keep += [nm, sh]
        arr[i].name = nm
        arr[i].ndim = len(shape)
        arr[i].shape = ctypes.cast(sh, ctypes.POINTER(ctypes.c_int64))
        arr[i].dtype = _lib.dtype_struct(dtype)
    return arr, keep


@dataclass
class TraceLayout:
    json_text: str
    total: int
    param_offsets: List[int]
    record_offsets: List[int]
    params: List[Tuple[str, Tuple[int, ...], str]]
    records: List[Tuple[str, Tuple[int, ...], str]]

    @staticmethod
    def compute(json_text: str, params, records) -> "TraceLayout":
        lib = _lib.load()
        pm, k1 = _metas(params)
        rm, k2 = _metas(records)
        po = (ctypes.c_int64 * max(1, len(params)))()
        ro = (ctypes.c_int64 * max(1, len(records)))()
        total = lib.tk_trace_layout(json_text.encode(), pm, len(params), rm, len(records), po, ro)
        if total < 0:
            _lib.check(int(total), "tk_trace_layout")
        return TraceLayout(json_text, int(total), list(po[:len(params)]), list(ro[:len(records)]),
                           list(params), list(records))

    def write_headers(self, image_ptr: int, image_size: int) -> None:
        lib = _lib.load()
        pm, k1 = _metas(self.params)
        rm, k2 = _metas(self.records)
        _lib.check(lib.tk_trace_write_headers(self.json_text.encode(), pm, len(self.params), rm, len(self.records),
                                              ctypes.c_void_p(image_ptr), image_size), "tk_trace_write_headers")


def head_layout(json_text: str, params) -> Tuple[TraceLayout, int]:
    """Layout of a trace file's head (header, json, params blob) and where its records section
    starts; the same for both file versions."""
    layout = TraceLayout.compute(json_text, params, [])
    return layout, layout.total - int(_lib.load().tk_ndlist_layout(None, 0, None))


def save_ndarray_list(arrays: Dict[str, np.ndarray]) -> bytes:
    """NDArray-list blob (``SaveParams``, src/runtime/file_utils.cc:210-236) of host arrays, in
    insertion order, written through the C ABI (tk_ndlist_layout / tk_ndlist_write_headers)."""
    lib = _lib.load()
    items = [(k, tuple(np.asarray(v).shape), str(np.asarray(v).dtype)) for k, v in arrays.items()]
    metas, keep = _metas(items)
    offs = (ctypes.c_int64 * max(1, len(items)))()
    total = lib.tk_ndlist_layout(metas, len(items), offs)
    if total < 0:
        _lib.check(int(total), "tk_ndlist_layout")
    blob = bytearray(int(total))
    buf = (ctypes.c_char * len(blob)).from_buffer(blob)
    _lib.check(lib.tk_ndlist_write_headers(metas, len(items), buf, len(blob)), "tk_ndlist_write_headers")
    for i, v in enumerate(arrays.values()):
        raw = np.ascontiguousarray(v).reshape(-1).view(np.uint8)
        blob[offs[i]:offs[i] + raw.size] = raw.tobytes()
    return bytes(blob)


def header_json(meta: Dict[str, Any]) -> str:
    text = json.dumps(meta, separators=(",", ":"), sort_keys=False)
    return text + " " * JSON_SLACK


def write_file(path: str, image_ptr: int, size: int) -> None:
    _lib.check(_lib.load().tk_write_file(path.encode(), ctypes.c_void_p(image_ptr), size), "tk_write_file")


# ---------------------------------------------------------------- numpy reader

def _np_dtype(code: int, bits: int) -> np.dtype:
    kind = {0: "i", 1: "u", 2: "f"}[code]
    return np.dtype(f"<{kind}{bits // 8}")


def parse_ndarray_list(buf, offset: int = 0, size: Optional[int] = None, copy: bool = False) -> Dict[str, np.ndarray]:
    """Parse an NDArray-list blob (LoadParams, src/runtime/file_utils.cc:184-206)."""
    mv = memoryview(buf)
    end = len(mv) if size is None else offset + size
    off = offset

    def rd(fmt):
        nonlocal off
        n = struct.calcsize(fmt)
        if off + n > end:
            raise ValueError("truncated NDArray-list blob")
        v = struct.unpack_from(fmt, mv, off)
        off += n
        return v

    magic, _ = rd("<QQ")
    if magic != LIST_MAGIC:
        raise ValueError("not an NDArray-list blob")
    (n,) = rd("<Q")
    names = []
    for _ in range(n):
        (ln,) = rd("<Q")
        names.append(bytes(mv[off:off + ln]).decode())
        off += ln
    (na,) = rd("<Q")
    if na != n:
        raise ValueError("name/array count mismatch")
    out: Dict[str, np.ndarray] = {}
    for name in names:
        amagic, _, dev_type, dev_id, ndim = rd("<QQiii")
        if amagic != ARRAY_MAGIC:
            raise ValueError("bad array magic")
        code, bits, lanes = rd("<BBH")
        shape = rd(f"<{ndim}q") if ndim else ()
        (nbytes,) = rd("<q")
        dt = _np_dtype(code, bits)
        arr = np.frombuffer(mv, dtype=dt, count=nbytes // dt.itemsize, offset=off).reshape(shape)
        out[name] = arr.copy() if copy else arr
        off += nbytes
    return out


@dataclass
class Trace:
    meta: Dict[str, Any]
    params: Dict[str, np.ndarray]
    records: Dict[str, np.ndarray]


def _open(path_or_bytes):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview, mmap.mmap)):
        return path_or_bytes
    with open(path_or_bytes, "rb") as f:
        if os.fstat(f.fileno()).st_size == 0:
            raise ValueError("not a tachikoma trace (empty file)")
        return mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)


def _header(buf):
    if len(buf) < 56:
        raise ValueError("not a tachikoma trace (shorter than its header)")
    magic, version, jl, po, ps, ro, rs = struct.unpack_from("<7Q", buf, 0)
    if magic != TRACE_MAGIC:
        raise ValueError("not a tachikoma trace (bad magic)")
    return version, jl, po, ps, ro, rs


def read_trace(path_or_bytes, copy: bool = False) -> Trace:
    """The trace of a file of either version (a packed file is expanded first: unpack_trace)."""
    buf = _open(path_or_bytes)
    version, jl, po, ps, ro, rs = _header(buf)
    if version in PACKED_VERSIONS:
        buf = unpack_trace(buf)
        version, jl, po, ps, ro, rs = _header(buf)
    if version != TRACE_VERSION:
        raise ValueError(f"unsupported trace version {version}")
    meta = json.loads(bytes(buf[56:56 + jl]).decode())
    params = parse_ndarray_list(buf, po, ps, copy=copy)
    records = parse_ndarray_list(buf, ro, rs, copy=copy)
    return Trace(meta, params, records)


# ---------------------------------------------------------------- digests
# Host twin of the device digest (tk_digest_bytes, csrc/tk_trace.hip):
#   D(bytes) = Σ_i splitmix64_final(w_i ^ i·0x9E3779B97F4A7C15)  mod 2^64
# over little-endian 8-byte words w_i, the tail zero-padded.  The trace digest of a
# shard is D over the u64 array [D(record_0), D(record_1), ...] in record order, so
# it can be recomputed from a trace file without the GPU.

_PHI = np.uint64(0x9E3779B97F4A7C15)


def _mix64(z: np.ndarray) -> np.ndarray:
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def digest_bytes(buf, chunk_words: int = 1 << 22) -> int:
    raw = np.frombuffer(memoryview(buf).cast("B"), dtype=np.uint8)
    nw = (raw.size + 7) // 8
    total = np.uint64(0)
    full = raw.size // 8
    with np.errstate(over="ignore"):
        for s in range(0, nw, chunk_words):
            e = min(nw, s + chunk_words)
            if e <= full:
                w = raw[s * 8:e * 8].view("<u8")
            else:
                tail = np.zeros((e - s) * 8, np.uint8)
                part = raw[s * 8:]
                tail[:part.size] = part
                w = tail.view("<u8")
            idx = np.arange(s, e, dtype=np.uint64)
            total = total + np.sum(_mix64(w ^ (idx * _PHI)), dtype=np.uint64)
    return int(total)


def records_digest(records: "Dict[str, np.ndarray] | Sequence[np.ndarray]") -> int:
    """Digest of a shard's records in trace order (graph inputs first, then ops)."""
    arrays = list(records.values()) if isinstance(records, dict) else list(records)
    per = np.array([digest_bytes(np.ascontiguousarray(a).reshape(-1).view(np.uint8)) for a in arrays],
                   dtype=np.uint64)
    return digest_bytes(per.tobytes())


def trace_file_digest(path_or_bytes) -> int:
    """Digest of the records of a trace file of either version."""
    return records_digest(read_trace(path_or_bytes).records)


def trace_bytes(meta: Dict[str, Any], params: Dict[str, np.ndarray], records: Dict[str, np.ndarray]) -> bytes:
    """A complete trace file from host arrays (the same layout the device capture fills:
    tk_trace_layout / tk_trace_write_headers), e.g. for traces produced on the CPU."""
    p_items = [(k, tuple(np.asarray(v).shape), str(np.asarray(v).dtype)) for k, v in params.items()]
    r_items = [(k, tuple(np.asarray(v).shape), str(np.asarray(v).dtype)) for k, v in records.items()]
    layout = TraceLayout.compute(header_json(meta), p_items, r_items)
    blob = bytearray(layout.total)
    buf = (ctypes.c_char * len(blob)).from_buffer(blob)
    layout.write_headers(ctypes.addressof(buf), len(blob))
    del buf
    for offs, arrays in ((layout.param_offsets, params.values()), (layout.record_offsets, records.values())):
        for off, v in zip(offs, arrays):
            raw = np.ascontiguousarray(v).reshape(-1).view(np.uint8)
            blob[off:off + raw.size] = raw.tobytes()
    return bytes(blob)


# ---------------------------------------------------------------- packed trace files (version 2)
# A packed file holds the records in the trace wire coding (include/tachikoma.h, "wire format")
# instead of the NDArray-list blob.  Header, json and params blob are those of the version-1 file of
# the same run (only `version` and `records_size` differ); the records section is
#
#     u32 "TKPK" | u32 n_records | u64 plan_len | u64 wire_size | u64 raw_size
#     plan       one entry per record, in trace order:
#                u16 name_len, name, u8 dtype code, u8 dtype bits, u8 ndim, u8 coding, u8 diff,
#                ndim x i64 shape, and for a raw record u64 offset, u64 size (within the raw part)
#     pad to 8
#     wire       what tk_wire_encode_host writes for the coded records, in trace order
#     raw        the payloads of the records the wire does not code
#
# coding is the wire kind (0 int32, 1 int8, 2 uint8) or RAW; diff says the record is differenced
# against (int32) or clamp-predicted from (1-byte) the record before it.  The reader follows the
# stored plan and never calls plan_records, so the rule below may change without breaking a file.
# Nothing is padded beyond 8 bytes: a packed file is never larger than the version-1 file plus the
# wire's worst case (tk_wire_bound) minus the bytes of the coded records.

# Version 3 adds the bias coding of the wire (coding 3: an int32 record coded as the record before
# it plus a per-channel addend, include/tachikoma.h).  It is opt-in (pack_trace(bias=True),
# GraphModule.dump_trace(packed=True, bias=True)); the section header grows by one field and the
# addend values lie in the file, in a part of their own in front of the wire:
#
#     u32 "TKPK" | u32 n_records | u64 plan_len | u64 wire_size | u64 raw_size | u64 addend_size
#     plan       as version 2; an entry with coding 3 (dtype int32, diff 1) is followed by
#                u8 axis, u64 addend_off   (byte offset into the addends part, a multiple of 4)
#     pad to 8
#     addends    int32 values, channels = shape[axis] of them per coding-3 entry; padded to 8
#     wire       what tk_wire_encode_host_bias writes
#     raw
#
# `plane` is the product of the dims behind `axis`.  The file is self-contained: a reader follows the
# stored plan and the stored addend values and never looks at the graph or the params blob for them.

PACKED_VERSION = 2
PACKED_BIAS_VERSION = 3
PACKED_VERSIONS = (PACKED_VERSION, PACKED_BIAS_VERSION)
PACK_MAGIC = 0x4B504B54  # "TKPK"
RAW = 255
BIAS = 3  # coding of a bias-coded int32 record (version 3 only)
WIRE_KIND = {"int32": 0, "int8": 1, "uint8": 2}
_SECTION = struct.Struct("<IIQQQ")
_SECTION3 = struct.Struct("<IIQQQQ")


def _seg_kind(coding: int) -> int:
    """The element kind a coding's segments have: a bias-coded record is an int32 record."""
    return 0 if coding == BIAS else coding


def _align(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def _n_elems(shape) -> int:
    n = 1
    for d in shape:
        n *= int(d)
    return n


def plan_records(records: Sequence[Tuple[str, Sequence[int], str]]) -> List[Tuple[int, int]]:
    """The planning rule of packed files, (coding, diff) per record, from the record list alone
    (dtype, shape, order): an int32 record is wire kind 0, differenced when the record before it is a
    coded int32 record of the same shape; an int8 / uint8 record is kind 1 / 2, clamp-predicted when
    the record before it has the same kind and shape (blocks the clamp does not reproduce escape to a
    raw plane, so no node attributes are needed); every other dtype, and an empty record, is RAW.
    Both packers (GraphModule.dump_trace(packed=True) on the device, pack_trace on the host) use it."""
    plan: List[Tuple[int, int]] = []
    for i, (_, shape, dtype) in enumerate(records):
        kind = WIRE_KIND.get(str(np.dtype(dtype)), RAW)
        if kind != RAW and not 1 <= _n_elems(shape) <= 1 << 40:
            kind = RAW
        diff = int(kind != RAW and i > 0 and plan[i - 1][0] == kind and
                   tuple(int(d) for d in records[i - 1][1]) == tuple(int(d) for d in shape))
        plan.append((kind, diff))
    return plan


@dataclass
class PackedEntry:
    name: str
    shape: Tuple[int, ...]
    dtype: str
    coding: int
    diff: int
    raw_off: int = 0
    raw_size: int = 0
    axis: int = 0          # coding 3: the bias axis, and where its addend lies in the addends part
    addend_off: int = 0

    @property
    def nbytes(self) -> int:
        return _n_elems(self.shape) * np.dtype(self.dtype).itemsize

    @property
    def channels(self) -> int:
        return int(self.shape[self.axis])

    @property
    def plane(self) -> int:
        return _n_elems(self.shape[self.axis + 1:])


def packed_entries(records, plan=None, bias_axes=None) -> List[PackedEntry]:
    """Plan entries of a record list (raw payloads laid out in trace order).  ``bias_axes`` (version
    3): {record index: axis} of the records to bias-code, each of which the rule differences; their
    addends are laid out in trace order."""
    plan = plan_records(records) if plan is None else plan
    out, raw, add = [], 0, 0
    for i, ((name, shape, dtype), (coding, diff)) in enumerate(zip(records, plan)):
        e = PackedEntry(name, tuple(int(d) for d in shape), str(np.dtype(dtype)), int(coding), int(diff))
        if coding == RAW:
            e.raw_off, e.raw_size = raw, e.nbytes
            raw += e.raw_size
        if bias_axes and i in bias_axes:
            if (e.coding, e.diff) != (0, 1) or not 0 <= bias_axes[i] < len(e.shape) or _n_elems(e.shape) >= 1 << 31:
                raise ValueError(f"record {name} cannot be bias-coded: not a differenced int32 record of fewer than "
                                 f"2^31 elements with the axis {bias_axes[i]}")
            e.coding, e.axis, e.addend_off = BIAS, int(bias_axes[i]), add
            add += 4 * e.channels
        out.append(e)
    return out


def addend_bytes(entries: Sequence[PackedEntry]) -> int:
    """Size of the addends part of a version-3 file with these entries (padded to 8)."""
    return _align(sum(4 * e.channels for e in entries if e.coding == BIAS), 8)


def bias_axes_of_data(records: "Dict[str, np.ndarray]", plan=None) -> Tuple[Dict[int, int], Dict[int, np.ndarray]]:
    """The host packer's rule for the bias coding, ({record index: axis}, {record index: addend}).  It
    has no graph, so the rule is the data's: a record the version-2 rule differences, of rank >= 2
    and fewer than 2^31 elements, is bias-coded with axis 1 when ``rec - prev`` (int32 wrap-around)
    is constant over every (sample, channel) plane, with one constant per channel across all
    samples; that constant is the addend.  For a trace the engine wrote this selects every bias_add
    record (GraphModule.dump_trace(packed=True, bias=True) selects those by the graph), and others
    only for degenerate data: a record that happens to differ from the one before it by a constant
    per channel, e.g. where both are constant on every plane.  Any selection round-trips; it only
    decides how small the file is."""
    items = [(k, v.shape, str(v.dtype)) for k, v in records.items()]
    plan = plan_records(items) if plan is None else plan
    arrays = list(records.values())
    axes, addends = {}, {}
    for i, (coding, diff) in enumerate(plan):
        v = arrays[i]
        if (coding, diff) != (0, 1) or v.ndim < 2 or v.size >= 1 << 31:
            continue
        d = (v.view("<u4") - arrays[i - 1].view("<u4")).reshape(v.shape[0], v.shape[1], -1)
        add = d[0, :, 0]
        if np.array_equal(d, np.broadcast_to(add[None, :, None], d.shape)):
            axes[i], addends[i] = 1, add.view("<i4").copy()
    return axes, addends


def _plan_bytes(entries: Sequence[PackedEntry]) -> bytes:
    out = bytearray()
    for e in entries:
        nm = e.name.encode()
        d = _lib.dtype_struct(e.dtype)
        out += struct.pack("<H", len(nm)) + nm + struct.pack("<5B", d.code, d.bits, len(e.shape), e.coding, e.diff)
        out += struct.pack(f"<{len(e.shape)}q", *e.shape)
        if e.coding == RAW:
            out += struct.pack("<QQ", e.raw_off, e.raw_size)
        elif e.coding == BIAS:
            out += struct.pack("<BQ", e.axis, e.addend_off)
    return bytes(out)


def _parse_plan(mv, off: int, end: int, n: int, version: int = PACKED_VERSION) -> List[PackedEntry]:
    entries = []
    for _ in range(n):
        if off + 2 > end:
            raise ValueError("truncated coding plan")
        (ln,) = struct.unpack_from("<H", mv, off)
        off += 2
        if off + ln + 5 > end:
            raise ValueError("truncated coding plan")
        name = bytes(mv[off:off + ln]).decode()
        code, bits, ndim, coding, diff = struct.unpack_from("<5B", mv, off + ln)
        off += ln + 5
        extra = 16 if coding == RAW else 9 if coding == BIAS and version == PACKED_BIAS_VERSION else 0
        if off + 8 * ndim + extra > end:
            raise ValueError("truncated coding plan")
        shape = struct.unpack_from(f"<{ndim}q", mv, off)
        off += 8 * ndim
        if code not in (0, 1, 2) or bits not in (8, 16, 32, 64) or any(d < 0 for d in shape):
            raise ValueError(f"record {name}: bad dtype or shape in the coding plan")
        e = PackedEntry(name, tuple(shape), str(_np_dtype(code, bits)), coding, diff)
        if coding == RAW:
            e.raw_off, e.raw_size = struct.unpack_from("<QQ", mv, off)
            off += 16
        elif extra:
            e.axis, e.addend_off = struct.unpack_from("<BQ", mv, off)
            off += 9
        entries.append(e)
    return entries


def _wire_records(entries: Sequence[PackedEntry], offsets: Optional[Sequence[int]] = None):
    """tk_wire_record array of the coded entries (offsets: each entry's payload offset in the image)."""
    coded = [(e, o) for e, o in zip(entries, offsets or [0] * len(entries)) if e.coding != RAW]
    arr = (_lib.tk_wire_record * max(1, len(coded)))()
    for i, (e, o) in enumerate(coded):
        arr[i].offset, arr[i].n_elems, arr[i].diff, arr[i].kind = int(o), _n_elems(e.shape), e.diff, e.coding
    return arr, len(coded)


def _wire_addends(entries: Sequence[PackedEntry], base: int):
    """tk_wire_addend array beside _wire_records': the addends part starts at address ``base`` (host
    or device, as the entry point reads it)."""
    coded = [e for e in entries if e.coding != RAW]
    arr = (_lib.tk_wire_addend * max(1, len(coded)))()
    for i, e in enumerate(coded):
        if e.coding == BIAS:
            arr[i].plane, arr[i].channels, arr[i].addend = e.plane, e.channels, base + e.addend_off
    return arr


def wire_call(name: str, recs, addends, n: int, *rest, reader: bool = False) -> int:
    """The wire entry point ``name`` over ``recs`` (a packed file of version 2: ``addends`` None), or
    its twin that takes addends, ``name + "_bias"`` (version 3, with or without a bias-coded record).
    Returns what it returns; a failure is raised under the name of the entry point called
    (TachikomaError; for a ``reader`` of packed files the ValueError of a file that does not hold)."""
    lib = _lib.load()
    name, head = (name, (recs, n)) if addends is None else (name + "_bias", (recs, addends, n))
    rc = getattr(lib, name)(*head, *rest)
    if rc < 0 and reader:
        raise ValueError("packed trace: " + lib.tk_last_error().decode(errors="replace"))
    if rc < 0:
        _lib.check(int(rc), name)
    return int(rc)


@dataclass
class PackedPlan:
    """The records section of a packed file, from its entries and its version (2, or 3: a section
    header with ``addend_size`` and an addends part in front of the wire, whether or not an entry
    is bias-coded):  head | addends | wire | raw."""
    entries: List[PackedEntry]
    version: int = PACKED_VERSION

    def __post_init__(self):
        if self.version not in PACKED_VERSIONS:
            raise ValueError(f"not a packed trace version: {self.version}")
        self.bias = self.version == PACKED_BIAS_VERSION
        self.section = _SECTION3 if self.bias else _SECTION
        self.addend_size = addend_bytes(self.entries) if self.bias else 0
        self.raw_size = sum(e.raw_size for e in self.entries)

    def head(self, wire_size: int) -> bytes:
        """The section up to the addends part: section header, plan, pad to 8."""
        plan = _plan_bytes(self.entries)
        sizes = (wire_size, self.raw_size) + ((self.addend_size,) if self.bias else ())
        head = self.section.pack(PACK_MAGIC, len(self.entries), len(plan), *sizes) + plan
        return head + b"\0" * (_align(len(head), 8) - len(head))

    def size(self, wire_size: int) -> int:
        """Bytes of the whole section with a wire of ``wire_size`` (or of ``wire_bound()``)."""
        return len(self.head(wire_size)) + self.addend_size + wire_size + self.raw_size

    def wire_records(self, offsets: Optional[Sequence[int]] = None):
        """(tk_wire_record array, count) of the coded entries."""
        return _wire_records(self.entries, offsets)

    def wire_addends(self, base: int):
        """tk_wire_addend array for an addends part at address ``base``; None for version 2 (see wire_call)."""
        return _wire_addends(self.entries, base) if self.bias else None

    def wire_bound(self) -> int:
        """tk_wire_bound of the coded entries: the wire's size with every block raw (0: none coded)."""
        recs, n = self.wire_records()
        bound = int(_lib.load().tk_wire_bound(recs, n)) if n else 0
        if bound < 0:
            _lib.check(bound, "tk_wire_bound")
        return bound


def packed_section_head(entries: Sequence[PackedEntry], wire_size: int, version: int = PACKED_VERSION) -> bytes:
    """PackedPlan.head of the entries: the records section up to the wire or the addends part."""
    return PackedPlan(list(entries), version).head(wire_size)


def _ptr(buf) -> Tuple[int, np.ndarray]:
    a = np.frombuffer(buf, dtype=np.uint8)
    return a.ctypes.data, a


def pack_trace(path_or_bytes, bias: bool = False) -> bytes:
    """The host packer: the packed (version 2) file of a version-1 trace file, built on
    tk_wire_encode_host.  Compresses existing files without a GPU, and gives byte for byte what
    GraphModule.dump_trace(packed=True) writes for the same run.

    With ``bias`` the file is version 3: the records bias_axes_of_data selects (for a trace the
    engine wrote: the bias_add records; others only for degenerate data, see there) are bias-coded
    and their addends stored, and the file is byte for byte what
    GraphModule.dump_trace(packed=True, bias=True) writes wherever the two select the same records."""
    buf = _open(path_or_bytes)
    version, jl, po, ps, ro, rs = _header(buf)
    if version != TRACE_VERSION:
        raise ValueError(f"pack_trace wants a version-{TRACE_VERSION} trace, not version {version}")
    if not 56 + jl <= po <= po + ps <= ro <= ro + rs <= len(buf):
        raise ValueError("truncated trace file")
    records = parse_ndarray_list(buf, ro, rs)
    base, keep = _ptr(buf)
    items = [(k, v.shape, str(v.dtype)) for k, v in records.items()]
    offsets = [(v.ctypes.data - base) if v.size else ro for v in records.values()]
    axes, values = bias_axes_of_data(records) if bias else ({}, {})
    plan = PackedPlan(packed_entries(items, bias_axes=axes), PACKED_BIAS_VERSION if bias else PACKED_VERSION)
    entries = plan.entries
    addends = np.zeros(plan.addend_size // 4, "<i4")
    for i, v in values.items():
        addends[entries[i].addend_off // 4:entries[i].addend_off // 4 + v.size] = v
    recs, n = plan.wire_records(offsets)
    wire = b""
    if n:
        bound = plan.wire_bound()
        out = np.empty(bound, np.uint8)
        used = wire_call("tk_wire_encode_host", recs, plan.wire_addends(addends.ctypes.data), n, ctypes.c_void_p(base),
                         len(buf), ctypes.c_void_p(out.ctypes.data), bound)
        wire = out[:used].tobytes()
    raws = [v.tobytes() for e, v in zip(entries, records.values()) if e.coding == RAW]
    section = plan.head(len(wire)) + addends.tobytes() + wire + b"".join(raws)
    del keep
    return (struct.pack("<7Q", TRACE_MAGIC, plan.version, jl, po, ps, ro, len(section)) + bytes(buf[56:ro]) + section)


@dataclass
class PackedFile:
    """A parsed packed file: offsets are absolute."""
    json_text: str
    params_off: int
    params_size: int
    entries: List[PackedEntry]
    wire_off: int
    wire_size: int
    raw_off: int
    raw_size: int
    size: int
    version: int = PACKED_VERSION
    addend_off: int = 0    # version 3: the addends part (it ends where the wire starts)
    addend_size: int = 0   # as the file states it
    plan: Optional[PackedPlan] = None   # of ``entries`` and ``version``


def parse_packed(buf) -> PackedFile:
    """Header, sections and coding plan of a packed file (version 2 or 3), every extent checked
    against the buffer."""
    version, jl, po, ps, ro, rs = _header(buf)
    if version not in PACKED_VERSIONS:
        raise ValueError(f"not a packed (version {PACKED_VERSION} or {PACKED_BIAS_VERSION}) trace: version {version}")
    v3 = version == PACKED_BIAS_VERSION
    section = _SECTION3 if v3 else _SECTION
    size = len(buf)
    if not 56 + jl <= po <= po + ps <= ro <= ro + rs <= size or rs < section.size:
        raise ValueError("truncated packed trace file")
    try:
        json_text = bytes(buf[56:56 + jl]).decode()
        magic, n, plan_len, wire_size, raw_size, *rest = section.unpack_from(buf, ro)
        addend_size = rest[0] if rest else 0
        if magic != PACK_MAGIC:
            raise ValueError("packed trace: bad records section")
        addend_off = ro + _align(section.size + plan_len, 8)
        wire_off = addend_off + addend_size
        if wire_off + wire_size + raw_size != ro + rs or n > plan_len or addend_size % 8:
            raise ValueError("truncated packed trace file (sections do not add up)")
        entries = _parse_plan(memoryview(buf), ro + section.size, ro + section.size + plan_len, n, version)
    except (struct.error, UnicodeDecodeError) as e:
        raise ValueError(f"packed trace: {e}") from None
    for i, e in enumerate(entries):
        if e.coding == RAW:
            if e.raw_size != e.nbytes or e.raw_off + e.raw_size > raw_size:
                raise ValueError(f"record {e.name}: raw payload outside the file")
            continue
        before = entries[i - 1] if i else None
        if e.coding == BIAS and v3:
            if (e.diff != 1 or e.dtype != "int32" or not 1 <= _n_elems(e.shape) < 1 << 31 or before is None or
                    _seg_kind(before.coding) != 0 or _n_elems(before.shape) != _n_elems(e.shape)):
                raise ValueError(f"record {e.name}: bias coding of a record that is not a differenced int32 record of "
                                 f"fewer than 2^31 elements after a coded int32 record of the same element count")
            if e.axis >= len(e.shape) or e.shape[e.axis] < 1:
                raise ValueError(f"record {e.name}: bias axis {e.axis} is not an axis of shape {list(e.shape)}")
            if e.addend_off % 4 or e.addend_off + 4 * e.channels > addend_size:
                raise ValueError(f"record {e.name}: its addends do not lie inside the addends part")
        elif (WIRE_KIND.get(e.dtype) != e.coding or not 1 <= _n_elems(e.shape) <= 1 << 40 or e.diff not in (0, 1) or
              (e.diff and (before is None or _seg_kind(before.coding) != e.coding or
                           _n_elems(before.shape) != _n_elems(e.shape)))):
            raise ValueError(f"record {e.name}: coding {e.coding} / diff {e.diff} does not fit the record list")
    return PackedFile(json_text, po, ps, entries, wire_off, wire_size, wire_off + wire_size, raw_size, size,
                      int(version), addend_off, addend_size, PackedPlan(entries, int(version)))


def unpack_trace(path_or_bytes) -> bytearray:
    """Exactly the version-1 file dump_trace writes for the same run, byte for byte (a bytearray: it
    compares equal to the file's bytes and is not copied again).  The version-1 layout and headers
    are a function of the json, the params blob and the plan's names / dtypes / shapes
    (tk_trace_layout / tk_trace_write_headers); the coded records are expanded by tk_wire_decode, as
    the stored plan says.  Raises ValueError on a truncated or corrupted file and reads nothing
    outside it."""
    buf = _open(path_or_bytes)
    pf = parse_packed(buf)
    params = parse_ndarray_list(buf, pf.params_off, pf.params_size)
    p_items = [(k, v.shape, str(v.dtype)) for k, v in params.items()]
    r_items = [(e.name, e.shape, e.dtype) for e in pf.entries]
    # a width-0 block spends 5 bytes on 256 int32 elements: nothing expands further than that
    if sum(e.nbytes for e in pf.entries) > 256 * pf.size + (1 << 20):
        raise ValueError("packed trace: the plan's records cannot come from a file this small")
    try:
        layout = TraceLayout.compute(pf.json_text, p_items, r_items)
    except _lib.TachikomaError as e:
        raise ValueError(f"packed trace: {e}") from None
    image = bytearray(layout.total)
    cbuf = (ctypes.c_char * len(image)).from_buffer(image)
    try:
        layout.write_headers(ctypes.addressof(cbuf), len(image))
        po = _align(56 + len(pf.json_text.encode()), TRACE_ALIGN)
        if po != pf.params_off or po + pf.params_size > len(image):
            raise ValueError("packed trace: the params blob does not lie where the header says")
        image[po:po + pf.params_size] = buf[pf.params_off:pf.params_off + pf.params_size]
        recs, n = pf.plan.wire_records(layout.record_offsets)
        if n:
            base, keep = _ptr(buf)
            # (the addends part is 8-byte aligned in the file; mapped or copied, in memory too)
            wire_call("tk_wire_decode", recs, pf.plan.wire_addends(base + pf.addend_off), n,
                      ctypes.c_void_p(base + pf.wire_off), pf.wire_size, ctypes.c_void_p(ctypes.addressof(cbuf)),
                      len(image), 0, reader=True)
            del keep
        elif pf.wire_size:
            raise ValueError("packed trace: a wire buffer without coded records")
        for e, off in zip(pf.entries, layout.record_offsets):
            if e.coding == RAW:
                image[off:off + e.raw_size] = buf[pf.raw_off + e.raw_off:pf.raw_off + e.raw_off + e.raw_size]
    finally:
        del cbuf
    return image


@dataclass
class CheckedTrace:
    """A trace file of either version that passed check_trace: where its parts lie (absolute
    offsets) and how its records are stored.  ``entries`` are in trace order; in a version-1 file
    every entry is RAW with ``raw_off`` counted from ``records_off`` (the NDArray-list blob)."""
    version: int
    meta: Dict[str, Any]
    entries: List[PackedEntry]
    params: List[Tuple[str, Tuple[int, ...], str, int]]   # name, shape, dtype, absolute payload offset
    params_off: int
    params_size: int
    records_off: int      # packed: the wire's first byte (version 3: the addends part's); version 1: the records blob
    records_size: int     # packed: [addends +] wire + raw; version 1: the blob
    wire_size: int        # 0 in a version-1 file
    size: int
    addend_size: int = 0  # version 3: the addends part, which the wire follows

    @property
    def packed(self) -> bool:
        return self.version in PACKED_VERSIONS


def _list_items(buf, off: int, size: int):
    """(name, shape, dtype, absolute payload offset) of every array of an NDArray-list blob."""
    base, keep = _ptr(buf)
    out = []
    for k, v in parse_ndarray_list(buf, off, size).items():
        out.append((k, tuple(int(d) for d in v.shape), str(v.dtype), (v.ctypes.data - base) if v.size else off))
    del keep
    return out


def check_trace(buf, records, params=None) -> CheckedTrace:
    """Everything the host decides about a trace file before a byte of it goes to the device
    (GraphModule.verify_trace / load_trace): ``buf`` holds the whole file.  The header and the
    sections are parsed with every extent checked; a packed file's wire section must pass
    tk_wire_check, which is the gate of the device decoder; and the file's record list (names,
    dtypes, shapes, order) must equal ``records``, a list of (name, shape, dtype) -- a graph's
    plan.records -- and likewise its params where ``params`` is given.  ValueError otherwise: a
    truncated file, a plan or a wire table that does not hold, or a trace of another graph (or of
    another batch size, which is another record list)."""
    version = _header(buf)[0]
    addend_size = 0
    if version in PACKED_VERSIONS:
        pf = parse_packed(buf)
        try:
            meta = json.loads(pf.json_text)
        except ValueError:
            raise ValueError("packed trace: the header json does not parse") from None
        entries, po, ps = pf.entries, pf.params_off, pf.params_size
        recs, n = pf.plan.wire_records()
        if n:
            base, keep = _ptr(buf)
            wire_call("tk_wire_check", recs, pf.plan.wire_addends(base + pf.addend_off), n,
                      ctypes.c_void_p(base + pf.wire_off), pf.wire_size, reader=True)
            del keep
        elif pf.wire_size:
            raise ValueError("packed trace: a wire buffer without coded records")
        addend_size = pf.addend_size
        records_off, records_size = pf.wire_off - addend_size, addend_size + pf.wire_size + pf.raw_size
        wire_size = pf.wire_size
    elif version == TRACE_VERSION:
        _, jl, po, ps, ro, rs = _header(buf)
        if not 56 + jl <= po <= po + ps <= ro <= ro + rs <= len(buf):
            raise ValueError("truncated trace file")
        try:
            meta = json.loads(bytes(buf[56:56 + jl]).decode())
            items = _list_items(buf, ro, rs)
        except (struct.error, UnicodeDecodeError, KeyError, TypeError) as e:
            raise ValueError(f"trace file: {e}") from None
        entries = [PackedEntry(k, shape, dtype, RAW, 0, off - ro, _n_elems(shape) * np.dtype(dtype).itemsize)
                   for k, shape, dtype, off in items]
        if any(e.raw_off + e.raw_size > rs for e in entries):
            raise ValueError("truncated trace file")
        records_off, records_size, wire_size = ro, rs, 0
    else:
        raise ValueError(f"unsupported trace version {version}")
    want = [(n, tuple(int(d) for d in s), str(np.dtype(d))) for n, s, d in records]
    have = [(e.name, e.shape, e.dtype) for e in entries]
    if have != want:
        at = next((i for i, (a, b) in enumerate(zip(have, want)) if a != b), min(len(have), len(want)))
        raise ValueError(f"trace is of another graph: {len(have)} records against the graph's {len(want)}, the first "
                         f"difference at record {at} ({have[at] if at < len(have) else None} in the file, "
                         f"{want[at] if at < len(want) else None} in the graph)")
    try:
        p_items = _list_items(buf, po, ps)
    except (struct.error, UnicodeDecodeError, KeyError, TypeError) as e:
        raise ValueError(f"trace file: {e}") from None
    if any(off + _n_elems(shape) * np.dtype(dtype).itemsize > po + ps for _, shape, dtype, off in p_items):
        raise ValueError("truncated trace file (params)")
    if params is not None:
        want_p = sorted((n, tuple(int(d) for d in s), str(np.dtype(d))) for n, s, d in params)
        if sorted(p[:3] for p in p_items) != want_p:
            raise ValueError("trace is of another graph: its params are not the graph's")
    return CheckedTrace(int(version), meta, list(entries), p_items, po, ps, records_off, records_size, wire_size, len(buf),
                        addend_size)


def packed_info(path_or_bytes) -> Dict[str, Any]:
    """Sizes and the coding plan of a packed file (``python -m tachikoma_amd.trace_format info``)."""
    pf = parse_packed(_open(path_or_bytes))
    coded = sum(e.nbytes for e in pf.entries if e.coding != RAW)
    info = {"version": pf.version, "file_bytes": pf.size, "records": len(pf.entries), "wire_bytes": pf.wire_size,
            "coded_record_bytes": coded, "raw_record_bytes": pf.raw_size,
            "plan": [dict({"name": e.name, "dtype": e.dtype, "shape": list(e.shape),
                           "coding": "raw" if e.coding == RAW else e.coding, "diff": e.diff},
                          **({"axis": e.axis} if e.coding == BIAS else {})) for e in pf.entries]}
    if pf.plan.bias:
        info["addend_bytes"] = pf.addend_size
    return info


# ---------------------------------------------------------------- per-record statistics
# Host twin of the device statistics (tk_record_stats, csrc/tk_stats.hip): what a calibration
# reduces a record to -- count, sum, min, max, the histogram of magnitude bit lengths and, for
# 1-byte records, the histogram of values.  Everything is an exact integer, so the device's
# result, a trace file's and a merge of either are equal, not close.

STATS_KIND = WIRE_KIND  # the dtypes the statistics cover, by element kind
STATS_BITS, STATS_VALUES = 33, 256
STATS_DTYPE = np.dtype([("count", "<u8"), ("sum", "<i8"), ("min", "<i4"), ("max", "<i4"),
                        ("bits", "<u8", (STATS_BITS,)), ("values", "<u8", (STATS_VALUES,))])
_I32_MAX, _I32_MIN = 2 ** 31 - 1, -2 ** 31


def _wrap_i64(x: int) -> int:
    return (int(x) + 2 ** 63) % 2 ** 64 - 2 ** 63


@dataclass
class RecordStats:
    """Statistics of one record over everything accumulated into it.  ``sum`` is modulo 2^64 (as
    ``np.sum(x, dtype=np.int64)`` wraps); while ``count == 0``, ``min`` / ``max`` are INT32_MAX /
    INT32_MIN.  ``bits[b]`` counts the elements whose magnitude has bit length b (0 for 0, 32 for
    INT32_MIN); ``values[v - dtype_min]`` counts the elements equal to v (1-byte dtypes; None for
    int32)."""
    name: str
    dtype: str
    count: int
    min: int
    max: int
    sum: int
    bits: np.ndarray
    values: Optional[np.ndarray]

    @staticmethod
    def empty(dtype: str, name: str = "") -> "RecordStats":
        dtype = str(np.dtype(dtype))
        if dtype not in STATS_KIND:
            raise ValueError(f"record statistics cover {sorted(STATS_KIND)}, not {dtype}")
        return RecordStats(name, dtype, 0, _I32_MAX, _I32_MIN, 0, np.zeros(STATS_BITS, np.uint64),
                           None if dtype == "int32" else np.zeros(STATS_VALUES, np.uint64))

    @staticmethod
    def from_struct(row, dtype: str, name: str = "") -> "RecordStats":
        """From one tk_record_stats entry (an element of a STATS_DTYPE array)."""
        dtype = str(np.dtype(dtype))
        return RecordStats(name, dtype, int(row["count"]), int(row["min"]), int(row["max"]), int(row["sum"]),
                           np.array(row["bits"], np.uint64),
                           None if dtype == "int32" else np.array(row["values"], np.uint64))

    @property
    def absmax(self) -> int:
        """Largest magnitude, a Python int (2^31 for INT32_MIN); 0 for no elements."""
        return max(abs(self.min), abs(self.max)) if self.count else 0

    @property
    def mean(self) -> float:
        return self.sum / self.count if self.count else float("nan")

    def bit_width(self, coverage: float = 1.0) -> int:
        """Bits that hold ``coverage`` of the elements: the smallest b with sum(bits[:b+1]) >=
        ceil(coverage * count), plus a sign bit when min < 0."""
        import math
        need = math.ceil(coverage * self.count)
        cum, b = 0, 0
        for b in range(STATS_BITS):
            cum += int(self.bits[b])
            if cum >= need:
                break
        return b + (1 if self.count and self.min < 0 else 0)

    def percentile_abs(self, q: float) -> int:
        """``np.partition(np.abs(x), k)[k]`` with k = int(count * q), from the value histogram:
        what find_scale_by_percentile takes of a 1-byte record.  As there, the magnitude is taken
        in the record's own dtype, where |-128| of an int8 record is -128."""
        if self.values is None:
            raise ValueError(f"percentile_abs needs the value histogram of a 1-byte record, {self.name or 'this'} "
                             f"is {self.dtype}")
        k = int(self.count * q)
        if not 0 <= k < self.count:
            raise ValueError(f"percentile_abs: q = {q} selects element {k} of {self.count}")
        v = [int(c) for c in self.values]
        if self.dtype == "int8":
            order = [(-128, v[0])] + [(a, (v[128 + a] + v[128 - a]) if a else v[128]) for a in range(128)]
        else:
            order = list(enumerate(v))
        cum = 0
        for a, c in order:
            cum += c
            if cum > k:
                return a
        raise ValueError("percentile_abs: the value histogram does not add up to count")

    def merge(self, other: "RecordStats") -> "RecordStats":
        """Statistics of both together (the arithmetic of the kernel's flush)."""
        if other.dtype != self.dtype:
            raise ValueError(f"merge: {self.name} is {self.dtype}, {other.name} is {other.dtype}")
        return RecordStats(self.name, self.dtype, self.count + other.count, min(self.min, other.min),
                           max(self.max, other.max), _wrap_i64(self.sum + other.sum), self.bits + other.bits,
                           None if self.values is None else self.values + other.values)

    def equals(self, other: "RecordStats") -> bool:
        """Every field but the name."""
        return (self.dtype == other.dtype and (self.count, self.min, self.max, self.sum) ==
                (other.count, other.min, other.max, other.sum) and np.array_equal(self.bits, other.bits) and
                (self.values is None) == (other.values is None) and
                (self.values is None or np.array_equal(self.values, other.values)))

    def to_json(self) -> Dict[str, Any]:
        """Python ints throughout: they survive beyond 2^53."""
        return {"name": self.name, "dtype": self.dtype, "count": int(self.count), "min": int(self.min),
                "max": int(self.max), "sum": int(self.sum), "bits": [int(b) for b in self.bits],
                "values": None if self.values is None else [int(v) for v in self.values]}

    @staticmethod
    def from_json(d: Dict[str, Any]) -> "RecordStats":
        return RecordStats(d["name"], d["dtype"], int(d["count"]), int(d["min"]), int(d["max"]), int(d["sum"]),
                           np.array(d["bits"], np.uint64),
                           None if d["values"] is None else np.array(d["values"], np.uint64))


def record_stats(array, name: str = "") -> RecordStats:
    """The statistics of one host array (int32, int8 or uint8), in numpy."""
    x = np.asarray(array)
    out = RecordStats.empty(str(x.dtype), name)
    x = x.reshape(-1)
    if x.size == 0:
        return out
    wide = x.astype(np.int64)
    out.count = int(x.size)
    out.min, out.max = int(wide.min()), int(wide.max())
    out.sum = int(np.sum(wide, dtype=np.int64))
    length = np.searchsorted(2 ** np.arange(32, dtype=np.int64), np.abs(wide), side="right")
    out.bits = np.bincount(length, minlength=STATS_BITS).astype(np.uint64)
    if out.values is not None:
        out.values = np.bincount(wide - int(np.iinfo(x.dtype).min), minlength=STATS_VALUES).astype(np.uint64)
    return out


def trace_stats(path_or_bytes) -> Dict[str, RecordStats]:
    """The statistics of every int32 / int8 / uint8 record of a trace file of either version, in
    trace order; records of other dtypes are skipped.  Needs no GPU."""
    return {k: record_stats(v, k) for k, v in read_trace(path_or_bytes).records.items() if str(v.dtype) in STATS_KIND}


def merge_stats_dicts(parts: Sequence[Dict[str, RecordStats]]) -> Dict[str, RecordStats]:
    """Name by name merge of several results (chunks, files, ranks), in first-seen order."""
    out: Dict[str, RecordStats] = {}
    for part in parts:
        for k, s in part.items():
            out[k] = out[k].merge(s) if k in out else s
    return out


def stats_to_json(stats: Dict[str, RecordStats]) -> Dict[str, Any]:
    return {k: s.to_json() for k, s in stats.items()}


def stats_from_json(d: Dict[str, Any]) -> Dict[str, RecordStats]:
    return {k: RecordStats.from_json(v) for k, v in d.items()}


def main(argv=None) -> int:
    import argparse
    p = argparse.ArgumentParser(prog="python -m tachikoma_amd.trace_format",
                                description="Pack, unpack or describe tachikoma trace files.")
    sub = p.add_subparsers(dest="cmd", required=True)
    for name, text in (("pack", "version-1 file -> packed file"), ("unpack", "packed file -> version-1 file")):
        q = sub.add_parser(name, help=text)
        q.add_argument("src")
        q.add_argument("dst")
        if name == "pack":
            q.add_argument("--bias", action="store_true",
                           help="write version 3: bias_add records coded as the record before them plus a per-channel "
                                "addend stored in the file")
    sub.add_parser("info", help="sizes and coding plan of a file").add_argument("src")
    sub.add_parser("stats", help="per-record statistics of the files, merged, as one JSON object").add_argument(
        "files", nargs="+")
    args = p.parse_args(argv)
    if args.cmd == "stats":
        print(json.dumps(stats_to_json(merge_stats_dicts([trace_stats(f) for f in args.files]))))
        return 0
    if args.cmd == "info":
        version = _header(_open(args.src))[0]
        info = packed_info(args.src) if version in PACKED_VERSIONS else \
            {"version": version, "file_bytes": os.path.getsize(args.src), "records": len(read_trace(args.src).records)}
        print(json.dumps(info, indent=1))
        return 0
    out = pack_trace(args.src, bias=args.bias) if args.cmd == "pack" else unpack_trace(args.src)
    with open(args.dst, "wb") as f:
        f.write(out)
    print(f"{args.src}: {os.path.getsize(args.src)} -> {args.dst}: {len(out)} bytes")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
