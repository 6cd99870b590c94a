"""The device side of trace files, which GraphModule (graph_executor.py) drives: the captures that write
them (TraceCapture, PackedCapture), the verifier that checks, loads and replays them (TraceVerifier and
its reports), the per-record statistics (StatsAccumulator) and the float statistics of a profile graph
(FloatStatsAccumulator)."""
from __future__ import annotations

import ctypes
import os
import struct
import time
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from .. import _lib, trace_format as tf
from ..relay.device_module import DeviceModule


def _as_bytes(t):
    import torch
    return t.reshape(-1).view(torch.uint8)


class _Capture:
    """What the two captures share: the run's meta, the pinned image of the file with its head
    (header, json, params blob: ``layout``) written, and the params section kept equal to the
    module's params.  ``size`` is the number of bytes of the image that are the file."""

    def __init__(self, module: DeviceModule, meta: Dict[str, Any]):
        self.module = module
        self.meta = dict(meta)
        self.params = [(t.name, t.shape, t.dtype) for t in module.plan.params]
        self.records = [(t.name, t.shape, t.dtype) for t in module.plan.records]
        self.size = 0

    def _make_image(self, layout: "tf.TraceLayout", nbytes: int) -> None:
        """The pinned image of ``nbytes`` with the head of ``layout`` in it."""
        import torch
        self.layout = layout
        self.image = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.ptr = self.image.data_ptr()
        layout.write_headers(self.ptr, layout.total)
        # params once, from the device copies (again after load_params: refresh_params)
        self.param_offsets = {p[0]: (off, p[1], p[2]) for p, off in zip(self.params, layout.param_offsets)}
        self.refresh_params(list(self.param_offsets))

    def _host_bytes(self, off: int, shape, dtype: str):
        """Byte view of a payload (NDArray-list payloads are not element-aligned)."""
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        return self.image[off:off + nbytes]

    def refresh_params(self, names) -> None:
        """Copy the named params' device buffers into the params section (synchronous)."""
        for name in names:
            off, shape, dtype = self.param_offsets[name]
            self._host_bytes(off, shape, dtype).copy_(_as_bytes(self.module.buffers[name]))

    def update_meta(self, **kw) -> None:
        """The json keeps the length it had when the capture was made."""
        import torch
        self.meta.update(kw)
        text = tf.header_json(self.meta).rstrip()
        if len(text) > len(self.layout.json_text):
            raise _lib.TachikomaError("trace header grew beyond its reserved slack")
        text = text.ljust(len(self.layout.json_text))
        self.layout.json_text = text
        self.image[56:56 + len(text)].copy_(torch.frombuffer(bytearray(text.encode()), dtype=torch.uint8))

    def write(self, path: str) -> None:
        tf.write_file(path, self.ptr, self.size)

    def bytes(self) -> memoryview:
        return memoryview(self.image.numpy())[:self.size]


class TraceCapture(_Capture):
    """Pinned host image of one trace shard; device→host copies land at final offsets."""

    def __init__(self, module: DeviceModule, meta: Dict[str, Any]):
        import torch
        super().__init__(module, meta)
        layout = tf.TraceLayout.compute(tf.header_json(self.meta), self.params, self.records)
        self._make_image(layout, layout.total)
        self.size = layout.total
        self.record_offsets = dict(zip([r[0] for r in self.records], layout.record_offsets))
        self.host_dst = module.host_dst_array({n: self.ptr + off for n, off in self.record_offsets.items()})
        self.capture_stream = torch.cuda.Stream(device=module.device)

    def capture_inputs(self, stream) -> None:
        """Copy the graph inputs (recorded first) on the capture stream."""
        import torch
        self.capture_stream.wait_stream(stream)
        with torch.cuda.stream(self.capture_stream):
            for t in self.module.plan.inputs:
                self._host_bytes(self.record_offsets[t.name], t.shape, t.dtype).copy_(
                    _as_bytes(self.module.buffers[t.name]), non_blocking=True)

    def synchronize(self) -> None:
        self.capture_stream.synchronize()


class PackedCapture(_Capture):
    """One packed (version 2) trace file in the making: a device wire buffer, the pinned staging the
    file is written from, and the device packer between them.

    The records are packed where they lie (tk_wire_pack_device, which tells the host how many bytes
    it used), the records the wire does not code are gathered behind the used prefix, and one copy
    moves both into the staging at their place in the file.  No trace image exists and the host
    decoder is not involved.  The staging is sized once from tk_wire_bound (head + worst-case wire +
    raw records), not grown on demand: the worst case is the records' own size plus 2 %, and a
    buffer that never moves can be written from while the other one fills.

    With ``bias`` the file is version 3: an int32 record that plan.ops declares the nn.bias_add
    (axis 1) of the record directly before it, with an int32 param of shape[1] values as its bias
    and fewer than 2^31 elements, is bias-coded; every other record keeps the version-2 rule.  The
    capture owns one device int32 buffer with all addends (at the front of the wire buffer),
    refreshed together with the params; the packer reads it (tk_wire_pack_device_bias) and the
    bytes of that very buffer are copied into the file's addends part on the pack's stream, so the
    encoder's values and the file's cannot differ."""

    @staticmethod
    def bias_records(plan) -> Dict[int, Tuple[int, str]]:
        """{record index: (axis, bias param name)} of the records the bias rule selects."""
        records = plan.records
        rule = tf.plan_records([(t.name, t.shape, t.dtype) for t in records])
        index = {t.name: i for i, t in enumerate(records)}
        params = {t.name: t for t in plan.params}
        out = {}
        for o in plan.ops:
            i = index[o.name]
            if o.op != "nn.bias_add" or rule[i] != (0, 1) or len(o.inputs) != 2 or o.attrs.get("axis") != 1:
                continue
            b = params.get(o.inputs[1])
            if (o.inputs[0] == records[i - 1].name and b is not None and b.dtype == "int32" and
                    tf._n_elems(b.shape) == int(o.out.shape[1]) and tf._n_elems(o.out.shape) < 1 << 31):
                out[i] = (1, b.name)
        return out

    def __init__(self, module: DeviceModule, meta: Dict[str, Any], bias: bool = False):
        import torch
        super().__init__(module, meta)
        chosen = self.bias_records(module.plan) if bias else {}
        self.section = tf.PackedPlan(tf.packed_entries(self.records, bias_axes={i: a for i, (a, _) in chosen.items()}),
                                  tf.PACKED_BIAS_VERSION if bias else tf.PACKED_VERSION)
        self.entries = self.section.entries
        # bias param name -> [(first int32 of its addend in the addends part, values)]
        self.addend_of: Dict[str, List[Tuple[int, int]]] = {}
        for i, (_, name) in chosen.items():
            self.addend_of.setdefault(name, []).append((self.entries[i].addend_off // 4, self.entries[i].channels))
        addend_room = (self.section.addend_size + 63) // 64 * 64  # on the device: the wire behind it is 64-byte aligned
        coded = [e for e in self.entries if e.coding != tf.RAW]
        self.raw = [e for e in self.entries if e.coding == tf.RAW]
        self.raw_bytes = self.section.raw_size
        self.recs, self.n_coded = self.section.wire_records()
        self.src = (ctypes.c_void_p * max(1, len(coded)))(*[module.buffers[e.name].data_ptr() for e in coded])
        self.bound = self.section.wire_bound()
        buf = torch.empty(addend_room + max(64, self.bound + self.raw_bytes), dtype=torch.uint8, device=module.device)
        self.addends, self.wire = buf[:addend_room], buf[addend_room:]
        self.addends.zero_()  # the addends part's pad to 8 goes into the file; the wire stays uninitialised
        self.ads = self.section.wire_addends(self.addends.data_ptr())
        # header, json and params blob are those of the version-1 file (laid out without records)
        layout, self.records_off = tf.head_layout(tf.header_json(self.meta), self.params)
        self.addend_off = self.records_off + len(self.section.head(0))
        self.wire_off = self.addend_off + self.section.addend_size
        self._make_image(layout, self.records_off + self.section.size(self.bound))
        self.copy_stream = torch.cuda.Stream(device=module.device)
        self.used = 0
        self.stats: Dict[str, float] = {}
        self._copy_events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))

    def refresh_params(self, names) -> None:
        """The params section, and the addends that are among ``names`` (synchronous)."""
        super().refresh_params(names)
        for name in names:
            for at, count in self.addend_of.get(name, ()):
                self.addends[4 * at:4 * (at + count)].copy_(_as_bytes(self.module.buffers[name]))
        if self.addend_of:
            # the copies above are device to device on the current stream: wait for them, as the copies
            # into the params blob have been waited for, so that a pack on any stream reads these values
            import torch
            torch.cuda.current_stream(self.module.device).synchronize()

    def pack(self, stream) -> int:
        """Pack the records of the run queued on ``stream`` and start the copy into the staging;
        returns the file's size.  Waits for the run (the packer reports its length to the host);
        when it returns the record buffers may be overwritten by work queued on ``stream``."""
        import torch
        stream.synchronize()
        t0 = time.perf_counter()
        used = tf.wire_call("tk_wire_pack_device", self.recs, self.ads, self.n_coded, self.src,
                            ctypes.c_void_p(self.wire.data_ptr()), self.bound,
                            ctypes.c_void_p(_lib.stream_handle(stream))) if self.n_coded else 0
        self.stats = {"pack_ms": (time.perf_counter() - t0) * 1e3}
        with torch.cuda.stream(stream):
            for e in self.raw:
                self.wire[used + e.raw_off:used + e.raw_off + e.raw_size].copy_(
                    _as_bytes(self.module.buffers[e.name]), non_blocking=True)
            if self.section.addend_size:  # the values the packer has just read, in stream order
                self.image[self.addend_off:self.wire_off].copy_(self.addends[:self.section.addend_size], non_blocking=True)
        self.copy_stream.wait_stream(stream)
        n = used + self.raw_bytes
        with torch.cuda.stream(self.copy_stream):
            self._copy_events[0].record(self.copy_stream)
            if n:
                self.image[self.wire_off:self.wire_off + n].copy_(self.wire[:n], non_blocking=True)
            self._copy_events[1].record(self.copy_stream)
        # the head's variable fields: version, records_size; the section (the copy lands behind it)
        head = self.image.numpy()
        head[8:16] = np.frombuffer(struct.pack("<Q", self.section.version), np.uint8)
        head[40:56] = np.frombuffer(struct.pack("<QQ", self.records_off, self.section.size(used)), np.uint8)
        head[self.records_off:self.addend_off] = np.frombuffer(self.section.head(used), np.uint8)
        self.used, self.size = used, self.wire_off + n
        return self.size

    def synchronize(self) -> None:
        self.copy_stream.synchronize()
        self.stats["copy_ms"] = self._copy_events[0].elapsed_time(self._copy_events[1])

    def write(self, path: str) -> None:
        t0 = time.perf_counter()
        super().write(path)
        self.stats["write_ms"] = (time.perf_counter() - t0) * 1e3


@dataclass
class Mismatch:
    """One record of a trace file that the module's buffer does not equal."""
    name: str
    op: str                       # the op that produced the record ("input" for a graph input)
    position: int                 # in trace order
    dtype: str
    shape: Tuple[int, ...]
    count: int                    # differing elements
    flat_index: int               # the first of them
    first_index: Tuple[int, ...]  # the same, unravelled
    node: int = -1                # replay_trace: index of the node that writes the record


class VerifyReport:
    """What GraphModule.verify_trace returns.  ``ok``: no record differs and the params are equal.
    ``mismatches`` are in trace order, which is a topological order, so ``first`` (the earliest, or
    None) is the first op whose recorded inputs all verified.  ``stats``: read_ms, upload_ms,
    run_ms, compare_ms, file_bytes, upload_bytes, uploads, packed."""

    def __init__(self, verifier, source, n_records, mismatches, params_differing, stats):
        self._verifier, self._source = verifier, source
        self.n_records = n_records
        self.mismatches: List[Mismatch] = mismatches
        self.params_differing: List[str] = params_differing
        self.params_equal = not params_differing
        self.ok = not mismatches and self.params_equal
        self.first: Optional[Mismatch] = mismatches[0] if mismatches else None
        self.stats = stats

    def detail(self, m: Mismatch):
        """(expected, got) at ``m.flat_index``: the file's value, through the host reader
        (trace_format.read_trace: the slow path, meant for a failure only), and the value in the
        module's buffer as it stands now (one small D2H copy)."""
        expected = tf.read_trace(self._source).records[m.name].reshape(-1)[m.flat_index]
        got = self._verifier.module.buffers[m.name].reshape(-1)[m.flat_index].item()
        return expected.item(), got

    def __repr__(self):
        return (f"VerifyReport(ok={self.ok}, n_records={self.n_records}, mismatched={len(self.mismatches)}, "
                f"first={self.first.name if self.first else None}, params_equal={self.params_equal})")


@dataclass
class FaultyOp:
    """One op of a replay that did not compute what the file says it did."""
    name: str                     # the record the op writes
    op: str                       # the op that produced it
    node: int                     # index of its node in the native module's node list
    place: int                    # index in the node's chain of records (0: the head op)
    count: int                    # differing elements
    flat_index: int               # the first of them
    first_index: Tuple[int, ...]  # the same, unravelled
    basis: str                    # "node": the record differs from what this engine computes from the
    #                               node's recorded inputs (the replay compare); "input": the record is
    #                               not the op of its own recorded input (the chain check)


@dataclass
class FaultyNode:
    """One node of a replay with at least one record that differs from the file."""
    node: int                  # index in the native module's node list
    kind: str                  # DeviceModule.node_kinds: "conv_block", "add_block", an op name, ...
    records: Tuple[str, ...]   # the node's records in chain order
    first: str                 # the first of them that differs
    ops: List[FaultyOp] = field(default_factory=list)  # the faulty ops of the node (ReplayReport.ops)


class ReplayReport(VerifyReport):
    """What GraphModule.replay_trace returns.  A mismatch here means "this record is not what this
    engine computes from the file's recorded inputs of its node": every node ran on what the file
    recorded, not on what the node before it computed, so a fault stays in the node it occurs in
    and an independent fault behind it is reported too.  Graph-input records are loaded, not
    computed, and are never listed.  ``nodes``: one FaultyNode per node with a differing record, in
    node order; ``first`` is the first faulty node's first differing record.  ``mismatches`` and
    ``nodes`` have the granularity of the node: within a fused node (conv -> bias_add -> requantize
    -> [add] -> [clip]) the ops read one another's values inside one kernel, so in ``mismatches`` a
    fault still runs down the chain from the op it occurs in.

    ``ops`` has the granularity of the op: one FaultyOp per faulty op, in trace order (also grouped
    per node in ``FaultyNode.ops``); without the params, ``ok == (not ops)``.  The head op of a node
    (conv, dense, the add of an add block; the only op of a pool, a cast or any node of an unfused
    build) is judged by the replay compare, basis "node".  Every other op of a fused chain is
    judged by the chain check (tk_module_check_chains), which ran on the file's records before any
    node did: the op is computed from its own recorded input and compared with its recorded output,
    basis "input", independently of the op before it (relay/replay.py: attribute_ops).  Consequences:
    a producer's wrong convolution whose tail is consistent with it is listed as the conv alone,
    though all of the node's records are in ``mismatches``; a second fault further down the same
    chain is listed too; a record corrupted in the file is not its op of its input, so it shows as
    its producer's fault, and, since the next op of the chain read it, possibly as its consumer's
    (where the corruption changes what the consumer computes) -- a corrupted file and a wrongly
    computed record cannot be told apart from the file alone.  With ``replay_trace(ops=False)`` the
    chain check is skipped and ``ops`` is empty.

    ``detail(m)`` gives the file's value and the recomputed one (the buffers hold the replayed
    values).  ``stats`` adds store_ms, shadow_ms, replay_ms (HIP events), shadows (the number of
    shadows rebuilt up front) and, with ops, chain_ms (HIP events around the chain check) to
    VerifyReport's."""

    def __init__(self, verifier, source, n_records, mismatches, params_differing, stats, nodes, ops=()):
        super().__init__(verifier, source, n_records, mismatches, params_differing, stats)
        self.nodes: List[FaultyNode] = nodes
        self.ops: List[FaultyOp] = list(ops)
        if nodes:
            self.first = next(m for m in mismatches if m.name == nodes[0].first)

    def __repr__(self):
        return (f"ReplayReport(ok={self.ok}, n_records={self.n_records}, mismatched={len(self.mismatches)}, "
                f"faulty_nodes={[n.node for n in self.nodes]}, faulty_ops={[o.name for o in self.ops]}, "
                f"first={self.first.name if self.first else None}, "
                f"params_equal={self.params_equal})")


class TraceVerifier:
    """Checks trace files against a module on the device: a pinned staging a file is read into and
    a device buffer its records section (packed: the wire and the raw payloads as they are; version
    1: the records blob) and params blob are uploaded to.  Both are sized once for the module --
    the file head plus tk_wire_bound plus the raw bytes, or the version-1 file, whichever is larger
    -- and reused across files.  Nothing is uploaded that trace_format.check_trace (tk_wire_check
    for the wire section) did not accept on the very bytes of the staging: a damaged file is a
    ValueError on the host and the device never sees it.  The expected records are never
    materialised: tk_wire_unpack_device compares the module's buffers against the wire as it
    decodes it, tk_compare_device_batch compares what the wire does not code."""

    ALIGN = 4096

    def __init__(self, module: DeviceModule, meta: Dict[str, Any]):
        self.module = module
        self.lib = module.lib
        plan = module.plan
        self.params = [(t.name, t.shape, t.dtype) for t in plan.params]
        self.records = [(t.name, t.shape, t.dtype) for t in plan.records]
        self.ops = {o.name: o.op for o in plan.ops}
        self.inputs = {t.name for t in plan.inputs}
        text = tf.header_json(meta)
        v1 = tf.TraceLayout.compute(text, self.params, self.records)
        records_off = tf.head_layout(text, self.params)[1]
        # sized for either packed version: the version-3 plan and addends of the records the graph's
        # rule selects (tk_wire_bound does not depend on the coding); a file that needs more grows it
        chosen = PackedCapture.bias_records(plan)
        packed = tf.PackedPlan(tf.packed_entries(self.records, bias_axes={i: a for i, (a, _) in chosen.items()}),
                               tf.PACKED_BIAS_VERSION)
        # a file of the same graph from another job may carry a longer json: two pages of slack
        self._alloc(max(v1.total, records_off + packed.size(packed.wire_bound())) + 2 * self.ALIGN)
        self.uploads = 0  # H2D copies issued so far

    def _alloc(self, size: int) -> None:
        import torch
        self.staging = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        # (the params blob and a version-3 file's addends part are each rounded up to ALIGN on the device)
        self.device = torch.empty(size + 2 * self.ALIGN, dtype=torch.uint8, device=self.module.device)
        self.host = self.staging.numpy()

    def _read(self, source) -> int:
        """The file's bytes into the staging; returns their count."""
        if isinstance(source, (bytes, bytearray, memoryview)):
            n = len(source)
            if n > len(self.host):
                self._alloc(n)
            self.host[:n] = np.frombuffer(source, np.uint8)
            return n
        with open(source, "rb", buffering=0) as f:
            n = os.fstat(f.fileno()).st_size
            if n > len(self.host):
                self._alloc(n)
            got = 0
            while got < n:
                k = f.readinto(memoryview(self.host)[got:n])
                if not k:
                    break
                got += k
            return got

    def stage(self, source):
        """Read and check on the host: (CheckedTrace, stats).  Raises ValueError; uploads nothing."""
        t0 = time.perf_counter()
        n = self._read(source)
        t1 = time.perf_counter()
        ct = tf.check_trace(self.host[:n], self.records, self.params)
        return ct, {"read_ms": (t1 - t0) * 1e3, "check_ms": (time.perf_counter() - t1) * 1e3, "file_bytes": n,
                    "packed": ct.packed}

    def upload(self, ct, stream, stats) -> None:
        """Params blob at the front of the device buffer, records section behind it (each at a
        4 KiB boundary, so a packed file's wire is 64-byte aligned): one H2D copy each."""
        import torch
        self.params_at = 0
        # (version 3: the addends part leads the records section; it is placed so that the wire
        # behind it is at a 4 KiB boundary all the same)
        self.wire_at = (ct.params_size + self.ALIGN - 1) // self.ALIGN * self.ALIGN + \
            (ct.addend_size + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.records_at = self.wire_at - ct.addend_size
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            for at, off, size in ((self.params_at, ct.params_off, ct.params_size),
                                  (self.records_at, ct.records_off, ct.records_size)):
                if size:
                    self.device[at:at + size].copy_(self.staging[off:off + size], non_blocking=True)
                    self.uploads += 1
            e1.record(stream)
        e1.synchronize()
        stats["upload_ms"] = e0.elapsed_time(e1)
        stats["upload_bytes"] = ct.params_size + ct.records_size
        stats["uploads"] = self.uploads

    def _expected_ptr(self, ct, e) -> int:
        """Device address of a raw entry's payload."""
        base = self.device.data_ptr() + self.wire_at
        return base + (ct.wire_size if ct.packed else 0) + e.raw_off

    def _wire_call(self, ct, names, mode, stream):
        """tk_wire_unpack_device over the coded records (version 3: tk_wire_unpack_device_bias, the
        addends read from the uploaded addends part), with a destination for ``names`` only; returns
        {name: (count, first)} in compare mode."""
        coded = [e for e in ct.entries if e.coding != tf.RAW]
        if not coded:
            return {}
        plan = tf.PackedPlan(ct.entries, ct.version)
        recs, n = plan.wire_records()
        dst = (ctypes.c_void_p * n)(*[self.module.buffers[e.name].data_ptr() if e.name in names else None for e in coded])
        report = (_lib.tk_wire_mismatch * n)()
        tf.wire_call("tk_wire_unpack_device", recs, plan.wire_addends(self.device.data_ptr() + self.records_at), n,
                     ctypes.c_void_p(self.device.data_ptr() + self.wire_at), ct.wire_size, dst, mode, report,
                     ctypes.c_void_p(_lib.stream_handle(stream)))
        return {e.name: (int(r.mismatches), int(r.first)) for e, r in zip(coded, report) if e.name in names}

    def _copy_raw(self, ct, names, stream) -> None:
        """Device-to-device copies of the raw entries in ``names`` into the module's buffers."""
        import torch
        with torch.cuda.stream(stream):
            for e in ct.entries:
                if e.coding == tf.RAW and e.name in names and e.raw_size:
                    at = self._expected_ptr(ct, e) - self.device.data_ptr()
                    _as_bytes(self.module.buffers[e.name]).copy_(self.device[at:at + e.raw_size], non_blocking=True)

    def store(self, ct, names, stream) -> None:
        """The file's records ``names`` into the module's buffers (after the last traced run's
        copies have read them: tk_module_wait_capture, as set_input does)."""
        self.module.wait_capture(stream)
        self._wire_call(ct, names, _lib.TK_WIRE_UNPACK_STORE, stream)
        self._copy_raw(ct, names, stream)

    def compare(self, ct, stream):
        """({record name: (count, first)} over all records, [names of differing params])."""
        names = {e.name for e in ct.entries}
        out = self._wire_call(ct, names, _lib.TK_WIRE_UNPACK_COMPARE, stream)
        pairs = [(e.name, self._expected_ptr(ct, e), self.module.buffers[e.name], e.raw_size, False)
                 for e in ct.entries if e.coding == tf.RAW]
        pbase = self.device.data_ptr() + self.params_at - ct.params_off
        for name, shape, dtype, off in ct.params:
            nbytes = tf._n_elems(shape) * np.dtype(dtype).itemsize
            pairs.append((name, pbase + off, self.module.buffers[name], nbytes, True))
        differing = []
        if pairs:
            n = len(pairs)
            exp = (ctypes.c_void_p * n)(*[p[1] for p in pairs])
            got = (ctypes.c_void_p * n)(*[p[2].data_ptr() for p in pairs])
            cnt = (ctypes.c_int64 * n)(*[p[3] // p[2].element_size() for p in pairs])
            es = (ctypes.c_int32 * n)(*[p[2].element_size() for p in pairs])
            report = (_lib.tk_wire_mismatch * n)()
            _lib.check(self.lib.tk_compare_device_batch(exp, got, cnt, es, n, report,
                                                        ctypes.c_void_p(_lib.stream_handle(stream))),
                       "tk_compare_device_batch")
            for p, r in zip(pairs, report):
                if p[4]:
                    if r.mismatches:
                        differing.append(p[0])
                else:
                    out[p[0]] = (int(r.mismatches), int(r.first))
        return out, differing

    def mismatches(self, ct, found) -> List[Mismatch]:
        out = []
        for pos, e in enumerate(ct.entries):
            count, first = found.get(e.name, (0, _lib.NO_MISMATCH))
            if count:
                idx = tuple(int(i) for i in np.unravel_index(first, e.shape)) if e.shape else ()
                out.append(Mismatch(e.name, "input" if e.name in self.inputs else self.ops.get(e.name, "?"), pos,
                                    e.dtype, e.shape, count, first, idx))
        return out


class StatsAccumulator:
    """Per-record statistics accumulated on the device (tk_stats_plan_run into device-resident
    tk_record_stats entries): ``add`` after each run merges the record buffers as they stand,
    with no synchronisation, so ``for batch in data: gm.run(**batch); acc.add()`` calibrates over
    a dataset without a record leaving the device.  ``result`` copies the entries out and
    synchronises.  ``skipped`` names the records whose dtype the kernel does not cover.  The
    device memory is released by ``close`` or when the module is closed."""

    def __init__(self, module: DeviceModule, plan):
        import torch
        self.module, self.plan = module, plan
        self.names, self.skipped = list(plan.names), list(plan.skipped)
        words = max(1, len(self.names)) * tf.STATS_DTYPE.itemsize // 8
        self._dev = torch.empty(words, dtype=torch.int64, device=module.device)
        self._host = torch.empty(words, dtype=torch.int64, pin_memory=True)
        self.reset()

    def _stream(self, stream=None):
        import torch
        return torch.cuda.current_stream(self.module.device) if stream is None else stream

    def _live(self) -> None:
        if self._dev is None or self.module.closed:
            raise _lib.TachikomaError("the statistics accumulator was closed (with its module)")

    def reset(self, stream=None) -> None:
        """Back to the identity (no elements), enqueued on the stream."""
        self._live()
        if self.names:
            _lib.check(self.module.lib.tk_record_stats_reset(
                ctypes.c_void_p(self._dev.data_ptr()), len(self.names),
                ctypes.c_void_p(_lib.stream_handle(self._stream(stream)))), "tk_record_stats_reset")

    def add(self, stream=None) -> None:
        """Merge the record buffers as they stand: one launch on ``stream`` (default: the current
        one, where the run was enqueued), nothing uploaded, nothing waited for."""
        self._live()
        if self.names:
            _lib.check(self.module.lib.tk_stats_plan_run(
                self.plan.handle, ctypes.c_void_p(self._dev.data_ptr()),
                ctypes.c_void_p(_lib.stream_handle(self._stream(stream)))), "tk_stats_plan_run")

    def copy_to(self, host, stream=None) -> None:
        """Enqueue the copy of the entries into ``host`` (a pinned int64 tensor of ``words``)."""
        import torch
        self._live()
        with torch.cuda.stream(self._stream(stream)):
            host.copy_(self._dev, non_blocking=True)

    @property
    def words(self) -> int:
        return int(self._host.numel())

    def decode(self, host) -> Dict[str, "tf.RecordStats"]:
        rows = host.numpy().view(tf.STATS_DTYPE)
        return {n: tf.RecordStats.from_struct(rows[i], d, n)
                for i, (n, d) in enumerate(zip(self.names, self.plan.dtypes))}

    def result(self, stream=None) -> Dict[str, "tf.RecordStats"]:
        """{name: RecordStats} of everything added since the last reset: one copy, one
        synchronisation."""
        s = self._stream(stream)
        self.copy_to(self._host, s)
        s.synchronize()
        return self.decode(self._host)

    def close(self) -> None:
        self._dev = None


@dataclass
class FloatRange:
    """One tk_float_range entry: ``count`` elements, ``nonfinite`` of them NaN or +-inf, ``min`` /
    ``max`` of the finite ones as np.float32 (+inf / -inf while there is none)."""
    count: int
    nonfinite: int
    min: np.float32
    max: np.float32


RANGE_DTYPE = np.dtype([("count", "<u8"), ("nonfinite", "<u8"), ("min", "<f4"), ("max", "<f4")])
DIGIT_BINS = 2048  # entries of a record's digit table (levels 1 and 2 use the first 1024)
# tk_kl_row, tk_kl_pick and tk_kl_candidate (include/tachikoma.h)
KL_MAX_PICKS = 32
KL_OK, KL_COUNT_OVERFLOW, KL_ALL_INF, KL_TOO_MANY = 0, 1, 2, 3
KL_ROW_DTYPE = np.dtype([("d", "<f8"), ("bound", "<f8"), ("ps", "<f4"), ("qs", "<f4"), ("p_zeros", "<i4"),
                         ("q_zeros", "<i4")])
KL_PICK_DTYPE = np.dtype([("status", "<i4"), ("count", "<i4"), ("idx", "<i4", (KL_MAX_PICKS,))])
KL_CANDIDATE_DTYPE = np.dtype([("div", "<f4"), ("ps", "<f4"), ("qs", "<f4"), ("p_zeros", "<i4"), ("q_zeros", "<i4")])


class FloatStatsAccumulator:
    """Float statistics accumulated on the device (tk_fstats_plan_* into device-resident results),
    for the float32 records of a profile graph: after each run ``add_range``, ``add_histogram`` or
    ``add_digits`` merges the record buffers as they stand -- one launch, nothing uploaded, nothing
    waited for -- and only ``ranges``, ``histograms`` and ``digits`` copy results out and
    synchronise.  The histogram follows np.histogram over the edges ``set_edges`` builds from the
    accumulated ranges; the digit counts serve an exact radix select of |x|
    (relay.quantize.passes.radix_select).  The device memory is released by ``close`` or when the
    module is closed."""

    def __init__(self, module: DeviceModule, plan):
        import torch
        self.module, self.plan = module, plan
        self.names = list(plan.names)
        self._n = max(1, len(self.names))
        self._ranges = torch.empty(self._n * RANGE_DTYPE.itemsize // 8, dtype=torch.int64, device=module.device)
        self._edges = self._hist = self._digits = self._prefix = None
        self._edges_host: Optional[np.ndarray] = None
        self._known: Optional[Dict[str, FloatRange]] = None  # the ranges as last read, None once they grew
        self._keep: List[Any] = []                           # pinned sources of uploads in flight
        self.bins = 0
        self._digit_key = None
        self._kl_table = None                 # device: the last kl_thresholds' rows
        self._kl_cand = 0
        self.kl_picks: Optional[np.ndarray] = None  # the last kl_thresholds' pick rows (KL_PICK_DTYPE, one per name)
        self.kl_fallbacks: List[str] = []     # the records the last kl_thresholds sent through kl_threshold
        self.reset_ranges()

    def _stream(self, stream=None):
        import torch
        return torch.cuda.current_stream(self.module.device) if stream is None else stream

    def _handle(self, stream) -> ctypes.c_void_p:
        return ctypes.c_void_p(_lib.stream_handle(self._stream(stream)))

    def _live(self) -> None:
        if self._ranges is None or self.module.closed:
            raise _lib.TachikomaError("the float statistics accumulator was closed (with its module)")

    def _upload(self, array: np.ndarray, dev, stream) -> None:
        import torch
        host = torch.from_numpy(np.ascontiguousarray(array).view(np.int32).reshape(-1)).pin_memory()
        self._keep = self._keep[-3:] + [host]
        with torch.cuda.stream(self._stream(stream)):
            dev.copy_(host, non_blocking=True)

    def _download(self, dev, stream) -> np.ndarray:
        import torch
        s = self._stream(stream)
        with torch.cuda.stream(s):
            host = dev.to("cpu", non_blocking=True)
        s.synchronize()
        return host.numpy()

    def reset_ranges(self, stream=None) -> None:
        """The ranges back to the identity (no elements), enqueued on the stream."""
        self._live()
        self._known = None
        if self.names:
            _lib.check(self.module.lib.tk_float_range_reset(ctypes.c_void_p(self._ranges.data_ptr()), len(self.names),
                                                            self._handle(stream)), "tk_float_range_reset")

    def add_range(self, stream=None) -> None:
        """Merge the records' ranges as the buffers stand: one launch on ``stream`` (default: the
        current one, where the run was enqueued)."""
        self._live()
        self._known = None
        if self.names:
            _lib.check(self.module.lib.tk_fstats_plan_range(self.plan.handle, ctypes.c_void_p(self._ranges.data_ptr()),
                                                            self._handle(stream)), "tk_fstats_plan_range")

    def ranges(self, stream=None) -> Dict[str, FloatRange]:
        """{name: FloatRange} of everything added since the last reset: one copy, one synchronisation."""
        self._live()
        rows = self._download(self._ranges, stream).view(RANGE_DTYPE)
        self._known = {n: FloatRange(int(r["count"]), int(r["nonfinite"]), np.float32(r["min"]), np.float32(r["max"]))
                       for n, r in zip(self.names, rows)}
        return dict(self._known)

    def set_edges(self, bins: int, stream=None) -> None:
        """Give every record numpy's own ``bins + 1`` float32 edges over (-thres, thres), thres the
        larger magnitude of its accumulated range (relay.quantize.passes.histogram_edges), upload
        them and zero the histograms.  Reads the ranges (``ranges()``) unless they were read since
        the last ``add_range``; a record without finite values is a ValueError."""
        import torch
        from ..relay.quantize.passes import histogram_edges
        self._live()
        if not 2 <= bins <= 8192:
            raise ValueError(f"set_edges: bins must lie in 2..8192, not {bins}")
        known = self._known if self._known is not None else self.ranges(stream)
        edges = np.zeros((self._n, bins + 1), np.float32)
        for i, name in enumerate(self.names):
            r = known[name]
            if r.nonfinite or not (np.isfinite(r.min) and np.isfinite(r.max)):
                raise ValueError(f"set_edges: record {name} has no finite range "
                                 f"({r.count} values, {r.nonfinite} of them NaN or infinite)")
            edges[i] = histogram_edges(r.min, r.max, bins)
        dev = self.module.device
        self.bins, self._edges_host = bins, edges
        self._edges = torch.empty(self._n * (bins + 1), dtype=torch.int32, device=dev)
        self._upload(edges, self._edges, stream)
        with torch.cuda.stream(self._stream(stream)):
            self._hist = torch.zeros(self._n * bins, dtype=torch.int64, device=dev)

    def add_histogram(self, stream=None) -> None:
        """Count the record buffers as they stand into the histograms: one launch on ``stream``."""
        self._live()
        if self._hist is None:
            raise ValueError("add_histogram: set_edges first")
        if self.names:
            _lib.check(self.module.lib.tk_fstats_plan_histogram(
                self.plan.handle, ctypes.c_void_p(self._edges.data_ptr()), self.bins,
                ctypes.c_void_p(self._hist.data_ptr()), self._handle(stream)), "tk_fstats_plan_histogram")

    def histograms(self, stream=None) -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
        """{name: (counts, edges)} as np.histogram returns them (uint64 counts, float32 edges) of
        everything added since ``set_edges``: one copy, one synchronisation."""
        self._live()
        if self._hist is None:
            raise ValueError("histograms: set_edges first")
        counts = self._download(self._hist, stream).view(np.uint64).reshape(self._n, self.bins)
        return {n: (counts[i].copy(), self._edges_host[i].copy()) for i, n in enumerate(self.names)}

    def add_digits(self, level: int, prefixes=None, stream=None) -> None:
        """Count one level of the radix select of |x| over the record buffers as they stand: one
        launch on ``stream``.  ``prefixes`` holds, per record in ``names`` order, the bits of |x|
        above the level's digit (None at level 0).  Calls with the same level and prefixes
        accumulate; another level or other prefixes zero the tables and upload the prefixes first."""
        import torch
        self._live()
        if level not in (0, 1, 2):
            raise ValueError(f"add_digits: level must be 0, 1 or 2, not {level}")
        pre = [0] * len(self.names) if prefixes is None else [int(p) for p in prefixes]
        if len(pre) != len(self.names):
            raise ValueError(f"add_digits: {len(pre)} prefixes for {len(self.names)} records")
        key = (level, tuple(pre))
        if key != self._digit_key:
            dev = self.module.device
            if self._prefix is None:
                self._prefix = torch.empty(self._n, dtype=torch.int32, device=dev)
                self._digits = torch.empty(self._n * DIGIT_BINS, dtype=torch.int64, device=dev)
            self._upload(np.array(pre + [0] * (self._n - len(pre)), np.uint32), self._prefix, stream)
            with torch.cuda.stream(self._stream(stream)):
                self._digits.zero_()
            self._digit_key = key
        if self.names:
            _lib.check(self.module.lib.tk_fstats_plan_digits(
                self.plan.handle, level, ctypes.c_void_p(self._prefix.data_ptr()),
                ctypes.c_void_p(self._digits.data_ptr()), self._handle(stream)), "tk_fstats_plan_digits")

    def digits(self, stream=None) -> Dict[str, np.ndarray]:
        """{name: uint64 counts per digit} of the level last added (2048 entries at level 0, 1024
        below): one copy, one synchronisation."""
        self._live()
        if self._digits is None:
            raise ValueError("digits: add_digits first")
        used = DIGIT_BINS if self._digit_key[0] == 0 else DIGIT_BINS // 2
        counts = self._download(self._digits, stream).view(np.uint64).reshape(self._n, DIGIT_BINS)
        return {n: counts[i, :used].copy() for i, n in enumerate(self.names)}

    def kl_thresholds(self, num_quantized_bins: int = 255, stream=None) -> Dict[str, float]:
        """{name: threshold} of relay.quantize's kl_divergence search over the accumulated
        histograms, equal to ``kl_threshold``'s on each of them, with the search done where the
        histograms lie (tk_kl_device): the device evaluates every candidate window as an interval
        that contains the host's float32 divergence and lists the candidates that can be the host's
        argmin; only those pick rows are downloaded.  A single survivor is the answer; several are
        evaluated on the host by MinimizeKL's own code (tk_kl_candidates), first minimum wins.  A
        record with more than KL_MAX_PICKS survivors or with no finite divergence goes through
        ``kl_threshold`` (named in ``kl_fallbacks``); a count above INT32_MAX is a ValueError.
        The pick rows stay in ``kl_picks``, the intervals are read by ``kl_table()``."""
        import torch
        from ..relay.quantize.passes import kl_threshold
        self._live()
        if self._hist is None:
            raise ValueError("kl_thresholds: set_edges first")
        bins, nq = self.bins, int(num_quantized_bins)
        if bins % 2 == 0 or not 3 <= bins <= 8191 or not 2 <= nq <= bins:
            raise ValueError(f"kl_thresholds: needs an odd number of bins in 3..8191 and 2..bins quantized bins, "
                             f"not {bins} and {nq}")
        n = len(self.names)
        self._kl_cand = bins // 2 + 1 - nq // 2
        self.kl_fallbacks = []
        self.kl_picks = np.zeros(0, KL_PICK_DTYPE)
        if not n:
            return {}
        dev = self.module.device
        with torch.cuda.stream(self._stream(stream)):
            self._kl_table = torch.empty(n * self._kl_cand * KL_ROW_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
            picks_dev = torch.empty(n * KL_PICK_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
        _lib.check(self.module.lib.tk_kl_device(
            ctypes.c_void_p(self._hist.data_ptr()), n, bins, nq, ctypes.c_void_p(self._kl_table.data_ptr()),
            ctypes.c_void_p(picks_dev.data_ptr()), self._handle(stream)), "tk_kl_device")
        self.kl_picks = self._download(picks_dev, stream).view(KL_PICK_DTYPE).copy()
        counts = None  # the histograms, read only if a record needs the host
        found: Dict[str, float] = {}
        for i, name in enumerate(self.names):
            status, count = int(self.kl_picks[i]["status"]), int(self.kl_picks[i]["count"])
            if status != KL_OK or count > 1:
                if counts is None:
                    counts = self._download(self._hist, stream).view(np.uint64).reshape(self._n, bins)
                hist = counts[i]
            if status == KL_COUNT_OVERFLOW:
                raise ValueError(f"calibrate: a histogram bin of record {name} holds {int(hist.max())} values, "
                                 "more than MinimizeKL's int32 counts take")
            if status != KL_OK:
                self.kl_fallbacks.append(name)
                found[name] = kl_threshold(hist, self._edges_host[i], -1.0, "int8", bins, nq)
                continue
            idx = self.kl_picks[i]["idx"][:count]
            k = int(idx[0])
            if count > 1:  # the host's own evaluation of the survivors, ascending, strict <
                rows = kl_candidates(hist, bins, nq, idx)
                k = int(idx[int(np.argmin(rows["div"]))])
            found[name] = float(self._edges_host[i][bins // 2 + nq // 2 + k + 1])
        return found

    def kl_table(self, stream=None) -> Dict[str, np.ndarray]:
        """{name: KL_ROW_DTYPE rows, one per candidate} of the last ``kl_thresholds``: the device's
        divergences, their bounds and the exact parts (for tests and diagnostics)."""
        self._live()
        if self._kl_table is None:
            raise ValueError("kl_table: kl_thresholds first")
        rows = self._download(self._kl_table, stream).view(KL_ROW_DTYPE).reshape(len(self.names), self._kl_cand)
        return {n: rows[i].copy() for i, n in enumerate(self.names)}

    def close(self) -> None:
        self._ranges = self._edges = self._hist = self._digits = self._prefix = self._kl_table = None
        self._keep = []


def kl_candidates(hist, num_bins: int, num_quantized_bins: int, cand) -> np.ndarray:
    """tk_kl_candidates: MinimizeKL's own evaluation (KL_CANDIDATE_DTYPE rows) of the listed
    candidates of one histogram of ``num_bins`` counts."""
    h = np.ascontiguousarray(hist, np.int32)
    c = np.ascontiguousarray(cand, np.int32)
    out = np.zeros(c.size, KL_CANDIDATE_DTYPE)
    _lib.check(_lib.load().tk_kl_candidates(h.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), num_bins,
                                            num_quantized_bins, c.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), c.size,
                                            ctypes.c_void_p(out.ctypes.data)), "tk_kl_candidates")
    return out
