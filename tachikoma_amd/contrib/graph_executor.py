"""``graph_executor.GraphModule`` surface (python/tvm/contrib/graph_executor.py:114-351)
plus the trace capture the reference only sketches (README.md:6,16) and the debug
executor's per-node dump (python/tvm/contrib/debugger/debug_executor.py:210-347).

    lib = relay.build(mod, target="mi355x", params=params)
    m = graph_executor.GraphModule(lib["default"](tachikoma_amd.rocm(0)))
    m.set_input("data", x); m.run(); y = m.get_output(0).numpy()
    m.dump_trace("model.tkt")             # every op output of the last run
    m.run(trace=True)                     # run with overlapped D2H capture
"""
from __future__ import annotations

import ctypes
import json
import os
import time
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from .. import _lib
from .. import trace_format as tf
from ..relay.device_module import DeviceModule


class NDArrayView:
    """What get_output returns: ``.numpy()`` like tvm.nd.NDArray."""

    def __init__(self, t):
        self._t = t

    def numpy(self) -> np.ndarray:
        return self._t.detach().cpu().numpy()

    @property
    def shape(self):
        return tuple(self._t.shape)

    @property
    def dtype(self):
        return str(self._t.dtype).replace("torch.", "")

    def torch(self):
        return self._t


def _as_bytes(t):
    import torch
    return t.reshape(-1).view(torch.uint8)


class TraceCapture:
    """Pinned host image of one trace shard; device→host copies land at final offsets."""

    def __init__(self, module: DeviceModule, meta: Dict[str, Any]):
        import torch
        self.module = module
        plan = module.plan
        params = [(t.name, t.shape, t.dtype) for t in plan.params]
        records = [(t.name, t.shape, t.dtype) for t in plan.records]
        self.meta = dict(meta)
        self.layout = tf.TraceLayout.compute(tf.header_json(self.meta), params, records)
        self.image = torch.empty(self.layout.total, dtype=torch.uint8, pin_memory=True)
        self.ptr = self.image.data_ptr()
        self.layout.write_headers(self.ptr, self.layout.total)
        # params once, from the device copies (again after load_params: refresh_params)
        self.param_offsets = {p[0]: (off, p[1], p[2]) for p, off in zip(params, self.layout.param_offsets)}
        self.refresh_params(list(self.param_offsets))
        self.record_offsets = dict(zip([r[0] for r in records], self.layout.record_offsets))
        self.host_dst = module.host_dst_array({n: self.ptr + off for n, off in self.record_offsets.items()})
        self.capture_stream = torch.cuda.Stream(device=module.device)

    def refresh_params(self, names) -> None:
        """Copy the named params' device buffers into the params section (synchronous)."""
        for name in names:
            off, shape, dtype = self.param_offsets[name]
            self._host_bytes(off, shape, dtype).copy_(_as_bytes(self.module.buffers[name]))

    def _host_bytes(self, off: int, shape, dtype: str):
        """Byte view of a payload (NDArray-list payloads are not element-aligned)."""
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        return self.image[off:off + nbytes]

    def update_meta(self, **kw) -> None:
        self.meta.update(kw)
        text = tf.header_json(self.meta)
        old = self.layout.json_text
        if len(text.rstrip()) > len(old):
            raise _lib.TachikomaError("trace header grew beyond its reserved slack")
        text = text.rstrip().ljust(len(old))
        self.layout.json_text = text
        self.image[56:56 + len(text)].copy_(__import__("torch").frombuffer(bytearray(text.encode()),
                                                                           dtype=__import__("torch").uint8))

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

    def write(self, path: str) -> None:
        tf.write_file(path, self.ptr, self.layout.total)

    def bytes(self) -> memoryview:
        return memoryview(self.image.numpy())


class PackedCapture:
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
        import ctypes
        import torch
        self.module = module
        self.lib = module.lib
        self.bias = bool(bias)
        plan = module.plan
        params = [(t.name, t.shape, t.dtype) for t in plan.params]
        records = [(t.name, t.shape, t.dtype) for t in plan.records]
        self.meta = dict(meta)
        chosen = self.bias_records(plan) if self.bias else {}
        self.entries = tf.packed_entries(records, bias_axes={i: a for i, (a, _) in chosen.items()})
        # bias param name -> [(first int32 of its addend in the addends part, values)]
        self.addend_of: Dict[str, List[Tuple[int, int]]] = {}
        for i, (_, name) in chosen.items():
            self.addend_of.setdefault(name, []).append((self.entries[i].addend_off // 4, self.entries[i].channels))
        self.addend_bytes = tf.addend_bytes(self.entries) if self.bias else 0
        self.addend_room = (self.addend_bytes + 63) // 64 * 64  # on the device: the wire behind it is 64-byte aligned
        # header, json and params blob are those of the version-1 file (laid out without records)
        self.layout, self.records_off = tf.head_layout(tf.header_json(self.meta), params)
        coded = [e for e in self.entries if e.coding != tf.RAW]
        self.raw = [e for e in self.entries if e.coding == tf.RAW]
        self.raw_bytes = sum(e.raw_size for e in self.raw)
        self.recs, self.n_coded = tf._wire_records(self.entries, [0] * len(self.entries))
        self.src = (ctypes.c_void_p * max(1, len(coded)))(*[module.buffers[e.name].data_ptr() for e in coded])
        self.bound = 0
        if self.n_coded:
            self.bound = int(self.lib.tk_wire_bound(self.recs, self.n_coded))
            if self.bound < 0:
                _lib.check(self.bound, "tk_wire_bound")
        self.section_head = len(tf.packed_section_head(self.entries, 0, self.addend_bytes if self.bias else None))
        self.addend_off = self.records_off + self.section_head
        self.wire_off = self.addend_off + self.addend_bytes
        buf = torch.empty(self.addend_room + max(64, self.bound + self.raw_bytes), dtype=torch.uint8, device=module.device)
        self.addends, self.wire = buf[:self.addend_room], buf[self.addend_room:]
        self.addends.zero_()  # the addends part's pad to 8 goes into the file; the wire stays uninitialised
        self.ads = tf._wire_addends(self.entries, self.addends.data_ptr()) if self.bias else None
        self.image = torch.empty(self.wire_off + self.bound + self.raw_bytes, dtype=torch.uint8, pin_memory=True)
        self.ptr = self.image.data_ptr()
        self.layout.write_headers(self.ptr, self.layout.total)
        self.param_offsets = {p[0]: (off, p[1], p[2]) for p, off in zip(params, self.layout.param_offsets)}
        self.refresh_params(list(self.param_offsets))
        self.copy_stream = torch.cuda.Stream(device=module.device)
        self.used = 0
        self.size = 0
        self.stats: Dict[str, float] = {}
        self._copy_events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))

    def refresh_params(self, names) -> None:
        """Copy the named params' device buffers into the params section (synchronous)."""
        for name in names:
            off, shape, dtype = self.param_offsets[name]
            nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
            self.image[off:off + nbytes].copy_(_as_bytes(self.module.buffers[name]))
            for at, count in self.addend_of.get(name, ()):
                self.addends[4 * at:4 * (at + count)].copy_(_as_bytes(self.module.buffers[name]))
        if self.addend_of:
            # the copies above are device to device on the current stream: wait for them, as the copies
            # into the params blob have been waited for, so that a pack on any stream reads these values
            import torch
            torch.cuda.current_stream(self.module.device).synchronize()

    def update_meta(self, **kw) -> None:
        """As TraceCapture.update_meta: the json keeps the length it had when the capture was made."""
        import torch
        self.meta.update(kw)
        text = tf.header_json(self.meta)
        old = self.layout.json_text
        if len(text.rstrip()) > len(old):
            raise _lib.TachikomaError("trace header grew beyond its reserved slack")
        text = text.rstrip().ljust(len(old))
        self.layout.json_text = text
        self.image[56:56 + len(text)].copy_(torch.frombuffer(bytearray(text.encode()), dtype=torch.uint8))

    def pack(self, stream) -> int:
        """Pack the records of the run queued on ``stream`` and start the copy into the staging;
        returns the file's size.  Waits for the run (the packer reports its length to the host);
        when it returns the record buffers may be overwritten by work queued on ``stream``."""
        import ctypes
        import struct
        import torch
        stream.synchronize()
        t0 = time.perf_counter()
        used = 0
        if self.n_coded and self.bias:
            used = int(self.lib.tk_wire_pack_device_bias(self.recs, self.ads, self.n_coded, self.src,
                                                         ctypes.c_void_p(self.wire.data_ptr()), self.bound,
                                                         ctypes.c_void_p(_lib.stream_handle(stream))))
            if used < 0:
                _lib.check(used, "tk_wire_pack_device_bias")
        elif self.n_coded:
            used = int(self.lib.tk_wire_pack_device(self.recs, self.n_coded, self.src,
                                                    ctypes.c_void_p(self.wire.data_ptr()), self.bound,
                                                    ctypes.c_void_p(_lib.stream_handle(stream))))
            if used < 0:
                _lib.check(used, "tk_wire_pack_device")
        self.stats = {"pack_ms": (time.perf_counter() - t0) * 1e3}
        with torch.cuda.stream(stream):
            for e in self.raw:
                self.wire[used + e.raw_off:used + e.raw_off + e.raw_size].copy_(
                    _as_bytes(self.module.buffers[e.name]), non_blocking=True)
            if self.addend_bytes:  # the values the packer has just read, in stream order
                self.image[self.addend_off:self.wire_off].copy_(self.addends[:self.addend_bytes], non_blocking=True)
        self.copy_stream.wait_stream(stream)
        n = used + self.raw_bytes
        with torch.cuda.stream(self.copy_stream):
            self._copy_events[0].record(self.copy_stream)
            if n:
                self.image[self.wire_off:self.wire_off + n].copy_(self.wire[:n], non_blocking=True)
            self._copy_events[1].record(self.copy_stream)
        # the head's variable fields: version, records_size; the section (the copy lands behind it)
        head = self.image.numpy()
        section = tf.packed_section_head(self.entries, used, self.addend_bytes if self.bias else None)
        version = tf.PACKED_BIAS_VERSION if self.bias else tf.PACKED_VERSION
        head[8:16] = np.frombuffer(struct.pack("<Q", version), np.uint8)
        head[40:56] = np.frombuffer(struct.pack("<QQ", self.records_off, len(section) + self.addend_bytes + n), np.uint8)
        head[self.records_off:self.addend_off] = np.frombuffer(section, np.uint8)
        self.used, self.size = used, self.wire_off + n
        return self.size

    def synchronize(self) -> None:
        self.copy_stream.synchronize()
        self.stats["copy_ms"] = self._copy_events[0].elapsed_time(self._copy_events[1])

    def write(self, path: str) -> None:
        t0 = time.perf_counter()
        tf.write_file(path, self.ptr, self.size)
        self.stats["write_ms"] = (time.perf_counter() - t0) * 1e3

    def bytes(self) -> memoryview:
        return memoryview(self.image.numpy())[:self.size]


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
        import torch
        self.module = module
        self.lib = module.lib
        plan = module.plan
        self.params = [(t.name, t.shape, t.dtype) for t in plan.params]
        self.records = [(t.name, t.shape, t.dtype) for t in plan.records]
        self.ops = {o.name: o.op for o in plan.ops}
        self.inputs = {t.name for t in plan.inputs}
        text = tf.header_json(meta)
        v1 = tf.TraceLayout.compute(text, self.params, self.records)
        head, records_off = tf.head_layout(text, self.params)
        # sized for either packed version: the version-3 plan and addends of the records the graph's
        # rule selects (tk_wire_bound does not depend on the coding); a file that needs more grows it
        entries = tf.packed_entries(self.records, bias_axes={i: a for i, (a, _) in PackedCapture.bias_records(plan).items()})
        recs, n = tf._wire_records(entries, [0] * len(entries))
        bound = int(self.lib.tk_wire_bound(recs, n)) if n else 0
        if bound < 0:
            _lib.check(bound, "tk_wire_bound")
        raw = sum(e.raw_size for e in entries)
        addends = tf.addend_bytes(entries)
        packed = records_off + len(tf.packed_section_head(entries, 0, addends)) + addends + bound + raw
        # a file of the same graph from another job may carry a longer json: two pages of slack
        self._alloc(max(v1.total, packed) + 2 * self.ALIGN)
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
        import ctypes
        coded = [e for e in ct.entries if e.coding != tf.RAW]
        if not coded:
            return {}
        recs, n = tf._wire_records(ct.entries, [0] * len(ct.entries))
        dst = (ctypes.c_void_p * n)(*[self.module.buffers[e.name].data_ptr() if e.name in names else None for e in coded])
        report = (_lib.tk_wire_mismatch * n)()
        wire = ctypes.c_void_p(self.device.data_ptr() + self.wire_at)
        if ct.version == tf.PACKED_BIAS_VERSION:
            ads = tf._wire_addends(ct.entries, self.device.data_ptr() + self.records_at)
            _lib.check(self.lib.tk_wire_unpack_device_bias(recs, ads, n, wire, ct.wire_size, dst, mode, report,
                                                           ctypes.c_void_p(_lib.stream_handle(stream))),
                       "tk_wire_unpack_device_bias")
        else:
            _lib.check(self.lib.tk_wire_unpack_device(recs, n, wire, ct.wire_size, dst, mode, report,
                                                      ctypes.c_void_p(_lib.stream_handle(stream))), "tk_wire_unpack_device")
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
        import ctypes
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


class BenchmarkResult:
    """Runtimes from benchmarking, in seconds (python/tvm/runtime/module.py:34-98): ``results``
    and their mean / std / median / min / max."""

    def __init__(self, results):
        self.results = list(results)
        self.mean = float(np.mean(self.results))
        self.std = float(np.std(self.results))
        self.median = float(np.median(self.results))
        self.min = float(np.min(self.results))
        self.max = float(np.max(self.results))

    def __repr__(self):
        return (f"BenchmarkResult(min={self.min}, mean={self.mean}, median={self.median}, max={self.max}, "
                f"std={self.std}, results={self.results})")

    def __str__(self):
        head = "".join(f"{h:^12} " for h in ("mean (ms)", "median (ms)", "max (ms)", "min (ms)", "std (ms)"))
        vals = "".join(f"{v * 1000:^12.4f} " for v in (self.mean, self.median, self.max, self.min, self.std))
        return f"Execution time summary:\n{head}\n{vals}\n"


def time_evaluator(fn, device, number: int, repeat: int, min_repeat_ms: int = 0,
                   limit_zero_time_iterations: int = 100, cooldown_interval_ms: int = 0,
                   repeats_to_cooldown: int = 1, device_timer: bool = True):
    """``WrapTimeEvaluator`` (src/runtime/profiling.cc): one warm-up call, then ``repeat``
    measurements of ``number`` back-to-back calls each (seconds per call).  A measurement shorter
    than ``min_repeat_ms`` is redone with ``number`` grown (x1.618 at least, to the count the last
    one implies, as the reference does); a zero-time one at most ``limit_zero_time_iterations``
    times.  Device timer: HIP events on the device's current stream around the calls (the
    reference's Timer on ROCm); else wall clock with a device synchronize on both sides."""
    import torch
    stream = torch.cuda.current_stream(device)
    fn()
    torch.cuda.synchronize(device)
    out = []
    for r in range(max(1, repeat)):
        n = max(1, int(number))
        zeros = 0
        while True:
            if device_timer:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(n):
                    fn()
                e1.record(stream)
                e1.synchronize()
                ms = e0.elapsed_time(e1)
            else:
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                for _ in range(n):
                    fn()
                torch.cuda.synchronize(device)
                ms = (time.perf_counter() - t0) * 1e3
            if ms <= 0.0 and zeros < limit_zero_time_iterations:
                zeros += 1
                continue
            if ms >= (min_repeat_ms or 0) or ms <= 0.0:
                break
            n = max(int(min_repeat_ms / (ms / n) + 1), int(n * 1.618))
        out.append(ms * 1e-3 / n)
        if cooldown_interval_ms and repeats_to_cooldown and (r + 1) % repeats_to_cooldown == 0:
            time.sleep(cooldown_interval_ms * 1e-3)
    return out


class GraphModule:
    def __init__(self, module: DeviceModule):
        self.module = module
        self.plan = module.plan
        self._capture: Optional[TraceCapture] = None
        self._packed: Optional[PackedCapture] = None
        self._packed_bias: Optional[PackedCapture] = None
        self._verifier: Optional[TraceVerifier] = None
        self._accumulators: List[StatsAccumulator] = []
        self._one_shot: Dict[tuple, StatsAccumulator] = {}
        self._meta = {"format": "tachikoma-trace", "version": tf.TRACE_VERSION, "model": "graph",
                      "target": "mi355x", "sample_offset": 0, "rank": 0, "world": 1,
                      "semantics": {"reference": "tvm llvm target without -mcpu", "requantize_compute_dtype":
                                    _compute_dtypes(self.plan), "rounding_default": "UPWARD"},
                      "inputs": [t.name for t in self.plan.inputs],
                      "params": [t.name for t in self.plan.params],
                      "outputs": list(self.plan.outputs),
                      "ops": [o.describe() for o in self.plan.ops]}
        if self.plan.inputs:
            self._meta["n_samples"] = int(self.plan.inputs[0].shape[0]) if self.plan.inputs[0].shape else 1

    def close(self) -> None:
        """Wait for the device, then release the native module and the pinned trace image.  Call it
        (or use the module as a context manager) before the process exits; an atexit hook closes
        any module left open (device_module.close_all)."""
        self.module.close()
        for acc in self._accumulators:
            acc.close()
        self._accumulators, self._one_shot = [], {}
        if self._capture is not None:
            self._capture.capture_stream.synchronize()
            self._capture = None
        for cap in (self._packed, self._packed_bias):
            if cap is not None:
                cap.copy_stream.synchronize()
        self._packed = self._packed_bias = None
        self._verifier = None

    def __enter__(self) -> "GraphModule":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    # -- reference surface -------------------------------------------------
    def set_input(self, key=None, value=None, **params):
        """graph_executor.py:166-197: ``key`` (name or input index) = ``value`` plus keyword
        params; every shape is checked before the first write, and the writes wait for the
        last traced run's copies (tk_module_wait_capture)."""
        vals = {}
        if key is not None:
            vals[self.plan.inputs[key].name if isinstance(key, int) else key] = value
        vals.update(params)
        self.module.set_inputs(vals)

    def run(self, trace: bool = False, **inputs):
        import torch
        if inputs:
            self.set_input(**inputs)
        stream = torch.cuda.current_stream(self.module.device)
        if trace:
            cap = self.trace_capture()
            cap.capture_inputs(stream)
            self.module.run(stream, cap.capture_stream, cap.host_dst)
        else:
            self.module.run(stream)

    def pick_run_mode(self, steps: int = 2) -> Dict[str, Any]:
        """Submission find step for traced runs on this host: times ``steps`` traced runs issued
        node by node from the host (tk_module_run) and as one replayed HIP graph
        (tk_module_run_graph), and keeps the faster.  On a healthy host the host-issued copies
        reach the SDMA rate and win by ~5 % (profiles/r03n_run_modes.txt); on a host that issues
        the ~300 calls of a step slowly, the graph's single launch does — but such hosts can be
        slow only intermittently (profiles/r03r_run_modes_slow_host.txt: 454 vs 186 op-traces/s
        on one box), which two timed steps may not catch, so bench.py and trace jobs default to the
        graph.  Results are identical either way."""
        import time
        import torch
        times = {}
        for use_graph in (False, True):
            self.module.use_graph = use_graph
            self.run(trace=True)  # warm-up (a graph run captures and instantiates here)
            self.trace_capture().synchronize()
            torch.cuda.synchronize(self.module.device)
            t0 = time.perf_counter()
            for _ in range(max(1, steps)):
                self.run(trace=True)
            self.trace_capture().synchronize()
            torch.cuda.synchronize(self.module.device)
            times[use_graph] = (time.perf_counter() - t0) / max(1, steps)
        self.module.use_graph = times[True] < times[False]
        return {"host_issued_ms": round(times[False] * 1e3, 2), "graph_ms": round(times[True] * 1e3, 2),
                "chosen": "graph" if self.module.use_graph else "host-issued"}

    def get_num_outputs(self) -> int:
        return len(self.plan.outputs)

    def get_input_index(self, name: str) -> int:
        """graph_executor.py:247-260: the input's index, -1 when no input has that name."""
        return next((i for i, t in enumerate(self.plan.inputs) if t.name == name), -1)

    def get_input_info(self):
        """graph_executor.py:262-287: ({input: shape}, {input: dtype}) of the graph inputs (the
        arg nodes that are not params)."""
        return ({t.name: tuple(int(d) for d in t.shape) for t in self.plan.inputs},
                {t.name: t.dtype for t in self.plan.inputs})

    def debug_get_output(self, node, out=None):
        """graph_executor.py:305-316: only the debug executor runs a graph up to a node."""
        raise NotImplementedError("Please use debugger.debug_executor as graph_executor instead.")

    def share_params(self, other: "GraphModule", params_bytes: bytes) -> None:
        """graph_executor.py:328-339 (GraphExecutor::ShareParams, graph_executor.cc:293-310): take
        the params named in ``params_bytes`` (only the names are read) from ``other``, a module of
        the same graph.  The reference aliases the other executor's storage; here each node's
        tensors are the module's own device buffers, bound into its native node list, so the values
        are copied device to device (no host round trip) and the buffers derived from them (packed
        MFMA weights, weight sums) re-derived.  Every name must be a param of both modules with the
        same shape and dtype, checked before the first copy."""
        names = list(tf.parse_ndarray_list(params_bytes, copy=False))
        mine = {t.name: t for t in self.plan.params}
        theirs = {t.name: t for t in other.plan.params}
        sel = {}
        for name in names:
            if name not in mine or name not in theirs:
                raise _lib.TachikomaError(f"share_params: {name} is not a param of both modules")
            a, b = mine[name], theirs[name]
            if tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype:
                raise _lib.TachikomaError(f"share_params: {name} is {b.dtype}{list(b.shape)} in the other module, "
                                          f"{a.dtype}{list(a.shape)} here")
            sel[name] = other.module.buffers[name]
        self.module.set_inputs(sel)
        for cap in (self._capture, self._packed, self._packed_bias):
            if cap is not None:
                cap.refresh_params([n for n in sel if n in cap.param_offsets])

    _FUNCTIONS = ("set_input", "run", "get_output", "get_input", "get_num_outputs", "get_num_inputs",
                  "load_params", "share_params", "get_input_index", "get_input_info", "debug_get_output")

    def __getitem__(self, key: str):
        """graph_executor.py:341-349: the module function ``key`` (module["run"]() etc.)."""
        if key not in self._FUNCTIONS:
            raise AttributeError(f"Module has no function '{key}'")
        return getattr(self, key)

    def benchmark(self, device=None, func_name: str = "run", repeat: int = 5, number: int = 5,
                  min_repeat_ms=None, limit_zero_time_iterations: int = 100, end_to_end: bool = False,
                  cooldown_interval_ms: int = 0, repeats_to_cooldown: int = 1, **kwargs) -> BenchmarkResult:
        """graph_executor.py:351-459: runtimes of ``func_name`` (seconds per call), ``repeat``
        results of ``number`` calls each, timed with device timers (HIP events) so that input
        transfers are not counted.  ``kwargs`` are set as inputs first (not timed).  With
        ``end_to_end`` every call also copies ``kwargs`` host -> device and the outputs back,
        timed by the wall clock."""
        from ..relay.device_module import _as_torch_device
        dev = self.module.device if device is None else _as_torch_device(device)
        min_ms = 0 if min_repeat_ms is None else min_repeat_ms
        if end_to_end:
            host = {k: np.asarray(v.numpy() if hasattr(v, "numpy") else v) for k, v in kwargs.items()}

            def call():
                if host:
                    self.set_input(**host)
                self.run()
                for i in range(self.get_num_outputs()):
                    self.get_output(i).numpy()
            return BenchmarkResult(time_evaluator(call, dev, number, repeat, min_ms, limit_zero_time_iterations,
                                                  cooldown_interval_ms, repeats_to_cooldown, device_timer=False))
        if kwargs:
            self.set_input(**kwargs)
        fn = self[func_name]
        return BenchmarkResult(time_evaluator(fn, dev, number, repeat, min_ms, limit_zero_time_iterations,
                                              cooldown_interval_ms, repeats_to_cooldown))

    def get_num_inputs(self) -> int:
        return len(self.plan.inputs)

    def get_input(self, key) -> NDArrayView:
        if isinstance(key, int):
            key = self.plan.inputs[key].name
        return NDArrayView(self.module.buffers[key])

    def get_output(self, index: int, out=None) -> NDArrayView:
        t = self.module.buffers[self.plan.outputs[index]]
        if out is not None:
            out[...] = t.cpu().numpy()
            return out
        return NDArrayView(t)

    def load_params(self, params_bytes: bytes) -> None:
        """``GraphModule.load_params`` (python/tvm/contrib/graph_executor.py:318-327 →
        GraphExecutor::LoadParams, graph_executor.cc:283-291): an NDArray-list blob
        (file_utils.cc:184-206).  Names that are not graph inputs or params are skipped, like
        the reference; every other entry must match its buffer's shape and dtype, and all of
        them are checked before the first buffer is written.  The build-time buffers derived
        from a param (packed MFMA weights and weight sums) are re-derived on the device, and the
        params section of the trace image is refreshed."""
        known = {t.name: t for t in list(self.plan.inputs) + list(self.plan.params)}
        sel = {}
        for name, arr in tf.parse_ndarray_list(params_bytes, copy=True).items():
            t = known.get(name)
            if t is None:
                continue
            if tuple(arr.shape) != tuple(t.shape) or str(arr.dtype) != t.dtype:
                raise _lib.TachikomaError(f"load_params: {name} is {arr.dtype}{list(arr.shape)}, "
                                          f"the graph expects {t.dtype}{list(t.shape)}")
            sel[name] = arr
        self.module.set_inputs(sel)
        for cap in (self._capture, self._packed, self._packed_bias):
            if cap is not None:
                cap.refresh_params([n for n in sel if n in cap.param_offsets])

    # -- trace / debug surface ---------------------------------------------
    def get_node_output(self, name: str) -> NDArrayView:
        return NDArrayView(self.module.buffers[name])

    def node_names(self) -> List[str]:
        return [o.name for o in self.plan.ops]

    def trace_capture(self) -> TraceCapture:
        if self._capture is None:
            self._capture = TraceCapture(self.module, self._meta)
        return self._capture

    def packed_capture(self, bias: bool = False) -> PackedCapture:
        if bias:
            if self._packed_bias is None:
                self._packed_bias = PackedCapture(self.module, self._meta, bias=True)
            return self._packed_bias
        if self._packed is None:
            self._packed = PackedCapture(self.module, self._meta)
        return self._packed

    def set_trace_meta(self, **kw) -> None:
        self._meta.update(kw)
        for cap in (self._capture, self._packed, self._packed_bias):
            if cap is not None:
                cap.update_meta(**kw)

    def dump_trace(self, path: str, sample_offset: Optional[int] = None, packed: bool = False,
                   bias: bool = False) -> str:
        """Write the trace of the last run (re-runs with capture if the last run was not traced).

        With ``packed`` the file is a packed (version 2) trace: the run is compute-only, the records
        are packed on the device (tk_wire_pack_device) and one copy moves the used prefix of the wire
        buffer and the records the wire does not code into pinned staging, which is written out; no
        trace image is captured and the host decoder is not used.  The staging is sized from
        tk_wire_bound when the first packed trace is dumped (PackedCapture), not grown on demand.
        trace_format.unpack_trace gives back exactly the file ``packed=False`` writes, and
        trace_format.pack_trace of that file gives exactly this one.

        With ``packed`` and ``bias`` the file is version 3: the bias_add records are coded as the
        record before them plus their bias, whose values the file stores (PackedCapture;
        tk_wire_pack_device_bias).  pack_trace(bias=True) of the unpacked file gives exactly this
        one wherever its data rule selects the same records, and every reader takes both versions."""
        import torch
        if bias and not packed:
            raise ValueError("dump_trace: bias coding is a coding of packed files (packed=True)")
        if sample_offset is not None:
            self.set_trace_meta(sample_offset=int(sample_offset))
        stream = torch.cuda.current_stream(self.module.device)
        if packed:
            cap = self.packed_capture(bias)
            self.module.run(stream)
            cap.pack(stream)
            cap.synchronize()
            cap.write(path)
            return path
        cap = self.trace_capture()
        cap.capture_inputs(stream)
        self.module.run(stream, cap.capture_stream, cap.host_dst)
        cap.synchronize()
        cap.write(path)
        return path

    def trace_verifier(self) -> TraceVerifier:
        if self._verifier is None:
            self._verifier = TraceVerifier(self.module, self._meta)
        return self._verifier

    def verify_trace(self, path_or_bytes, run: bool = True) -> VerifyReport:
        """Check a trace file of either version against this module, record by record, on the
        device.  The file is read into pinned staging and checked on the host
        (trace_format.check_trace: extents, the coding plan, tk_wire_check on the wire section, and
        that its record list is this graph's; ValueError otherwise, before anything is uploaded).
        One copy moves its records section to the device as it is, another its params.  With
        ``run`` the file's graph-input records are put into the module's input buffers (the
        decoder's store mode, after tk_module_wait_capture like set_input; the shadows conv nodes
        read are rebuilt by the run itself) and the module runs once, compute only; with
        ``run=False`` the buffers are compared as they stand.  Then tk_wire_unpack_device in
        compare mode checks every coded record against the wire without ever expanding it,
        tk_compare_device_batch the other records and the params."""
        import torch
        v = self.trace_verifier()
        ct, stats = v.stage(path_or_bytes)
        stream = torch.cuda.current_stream(self.module.device)
        v.upload(ct, stream, stats)
        t0 = time.perf_counter()
        if run:
            v.store(ct, {t.name for t in self.plan.inputs}, stream)
            self.module.run(stream)
            stream.synchronize()
        t1 = time.perf_counter()
        found, params_differing = v.compare(ct, stream)
        stats["run_ms"] = (t1 - t0) * 1e3
        stats["compare_ms"] = (time.perf_counter() - t1) * 1e3
        return VerifyReport(v, path_or_bytes, len(ct.entries), v.mismatches(ct, found), params_differing, stats)

    def replay_trace(self, path_or_bytes, ops: bool = True) -> ReplayReport:
        """Re-execute every op of a trace file from its recorded inputs and compare, on the device.
        Reading, the host checks and the upload are verify_trace's (a damaged file is a ValueError
        before anything reaches the device).  Then every record of the file is stored into the
        module's buffers (as load_trace does), the shadows whose source is a record are rebuilt in
        one launch (tk_conv2d_make_shadow_batch), the nodes run in the order of relay/replay.py
        (record-producing nodes in reverse, each after the helper nodes it needs:
        tk_module_run_order), and one compare pass over the whole file gives the verdict of every
        node at once (ReplayReport).  With ``ops`` the chain check (tk_module_check_chains) runs
        between the store pass and the node run, where the buffers hold the file's records, and the
        report lists the faulty ops (ReplayReport.ops).  The nodes compute with the module's own params and packed
        weights; the file's params are compared and reported as by verify_trace.  Afterwards the
        buffers hold the replayed values, not a run's: the next run() overwrites everything."""
        import torch
        v = self.trace_verifier()
        order, shadows = self.module.replay_plan()  # (UnsupportedError before anything is touched)
        ct, stats = v.stage(path_or_bytes)
        stream = torch.cuda.current_stream(self.module.device)
        v.upload(ct, stream, stats)
        t0 = time.perf_counter()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record(stream)
        v.store(ct, {e.name for e in ct.entries}, stream)
        ev[1].record(stream)
        chain = None
        if ops:
            ce = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ce[0].record(stream)
            chain = self.module.check_chains(stream)
            ce[1].record(stream)
            ev[1] = ce[1]
        self.module.rebuild_shadows(shadows, stream)
        ev[2].record(stream)
        self.module.run_order(order, stream)
        ev[3].record(stream)
        stream.synchronize()
        t1 = time.perf_counter()
        found, params_differing = v.compare(ct, stream)
        stats["shadow_ms"], stats["replay_ms"] = (ev[k].elapsed_time(ev[k + 1]) for k in (1, 2))
        stats["store_ms"] = ev[0].elapsed_time(ce[0] if ops else ev[1])
        if ops:
            stats["chain_ms"] = ce[0].elapsed_time(ce[1])
        stats["shadows"] = len(shadows)
        stats["run_ms"] = (t1 - t0) * 1e3
        stats["compare_ms"] = (time.perf_counter() - t1) * 1e3
        node_of = {r: i for i, recs in enumerate(self.module.node_records) for r in recs}
        mismatches = [m for m in v.mismatches(ct, found) if m.name not in v.inputs]
        for m in mismatches:
            m.node = node_of.get(m.name, -1)
        bad = {m.name for m in mismatches}
        nodes = [FaultyNode(i, self.module.node_kinds[i], tuple(recs), next(r for r in recs if r in bad))
                 for i, recs in enumerate(self.module.node_records) if any(r in bad for r in recs)]
        faulty = []
        if ops:
            from ..relay.replay import attribute_ops
            shapes = {e.name: e.shape for e in ct.entries}
            for o in attribute_ops([(i, recs) for i, recs in enumerate(self.module.node_records) if recs],
                                   {m.name: (m.count, m.flat_index) for m in mismatches}, chain):
                shape = shapes[o["name"]]
                idx = tuple(int(i) for i in np.unravel_index(o["first"], shape)) if shape else ()
                faulty.append(FaultyOp(o["name"], v.ops.get(o["name"], "?"), o["node"], o["place"], o["count"],
                                       o["first"], idx, o["basis"]))
            position = {e.name: k for k, e in enumerate(ct.entries)}
            faulty.sort(key=lambda o: position[o.name])
            by_node = {n.node: n for n in nodes}
            for o in faulty:
                if o.node in by_node:
                    by_node[o.node].ops.append(o)
        return ReplayReport(v, path_or_bytes, len(ct.entries), mismatches, params_differing, stats, nodes, faulty)

    def load_trace(self, path_or_bytes, shadows: bool = False) -> None:
        """Put a trace file's records into the module's record buffers (the reading and the checks
        of verify_trace, then the decoder's store mode and device-to-device copies), so that
        get_node_output(name) returns what the file recorded.  Params are left alone.  With
        ``shadows`` the shadows whose source is a record are rebuilt from the loaded records
        (tk_conv2d_make_shadow_batch), so that module.run_range from any node works on loaded
        data; without it the shadows and other buffers derived from records are NOT rebuilt.  The
        next run() overwrites every record."""
        import torch
        v = self.trace_verifier()
        ct, stats = v.stage(path_or_bytes)
        stream = torch.cuda.current_stream(self.module.device)
        v.upload(ct, stream, stats)
        v.store(ct, {e.name for e in ct.entries}, stream)
        if shadows:
            self.module.rebuild_shadows(None, stream)
        stream.synchronize()

    def stats_accumulator(self, names=None) -> StatsAccumulator:
        """A fresh accumulator over the records ``names`` (default: all of them): ``add()`` after
        each run, ``result()`` at the end (StatsAccumulator).  Its device memory lives until it or
        this module is closed."""
        acc = StatsAccumulator(self.module, self.module.stats_plan(names))
        self._accumulators.append(acc)
        return acc

    def record_stats(self, names=None) -> Dict[str, "tf.RecordStats"]:
        """{name: RecordStats} of the record buffers as they stand -- after run, load_trace or a
        replay -- computed on the device: one statistics launch, one copy, one synchronisation.
        Records of dtypes the kernel does not cover are left out (stats_accumulator(...).skipped
        lists them).  Equals trace_format.record_stats of each record's host copy."""
        key = None if names is None else tuple(names)
        acc = self._one_shot.get(key)
        if acc is None:
            acc = self._one_shot[key] = self.stats_accumulator(names)
        acc.reset()
        acc.add()
        return acc.result()

    def trace_digest(self) -> int:
        """u64 digest of the last run's records, computed on the device
        (equals trace_format.trace_file_digest of the dumped trace)."""
        import torch
        d = self.module.records_digest(torch.cuda.current_stream(self.module.device))
        return int(d.item()) & 0xFFFFFFFFFFFFFFFF

    def profile(self) -> Dict[str, float]:
        """Per-node device time in ms (GraphExecutorDebug::RunIndividual analogue)."""
        return self.module.run_profiled()

    def chrome_trace(self, path: str) -> None:
        """Chrome trace JSON in the debug executor's schema (debug_result.py:151-189)."""
        timings = self.profile()
        events, t = [], 0.0
        for name, ms in timings.items():
            us = ms * 1e3  # Chrome trace "ts" is in microseconds (debug_result.py:151-189)
            events.append({"name": name, "cat": "Op", "ph": "B", "ts": t, "pid": 1, "tid": 1})
            events.append({"name": name, "cat": "Op", "ph": "E", "ts": t + us, "pid": 1, "tid": 1})
            t += us
        with open(path, "w") as f:
            json.dump({"traceEvents": events, "displayTimeUnit": "ns"}, f)


def _compute_dtypes(plan) -> str:
    """The requantize compute dtype(s) the plan's ops were built with (the trace header's claim):
    "int64" (the pinned default), "float32" / "float64", or a "+"-joined list when mixed."""
    cds = sorted({o.attrs.get("compute_dtype", "int64") for o in plan.ops if "compute_dtype" in o.attrs})
    return "+".join(cds) if cds else "int64"


def create(lib_factory, dev=None) -> GraphModule:
    return GraphModule(lib_factory["default"](dev))
