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

import json
import time
from typing import Any, Dict, List, Optional

import numpy as np

from .. import _lib
from .. import trace_format as tf
from ..relay.device_module import DeviceModule
from .trace_device import (FaultyNode, FaultyOp, FloatStatsAccumulator, Mismatch, PackedCapture,  # noqa: F401
                           ReplayReport, StatsAccumulator, TraceCapture, TraceVerifier, VerifyReport)


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

    def float_stats_accumulator(self, names=None) -> FloatStatsAccumulator:
        """A fresh float statistics accumulator over the float32 records ``names`` (default: all
        of them): ranges, edge histograms and radix-select digit counts kept on the device
        (FloatStatsAccumulator).  Its device memory lives until it or this module is closed."""
        acc = FloatStatsAccumulator(self.module, self.module.float_stats_plan(names))
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
