"""Device-side module: HBM buffers + the native node list (tk_module).

Memory layout in HBM (one GPU, one batch shard):
  * params: uploaded once; MFMA convs additionally hold a packed
    [Cout_pad][KH][KW][Cin_pad] int8 copy and int32 per-channel weight sums;
  * graph inputs and EVERY op output get their own buffer (no storage-pool
    reuse as in graph_executor.cc:356-464), so each output stays addressable
    for the trace copy-out until the step ends — ResNet-50 at 64 samples is
    ~7 GB, nothing next to 288 GB;
  * every tensor read by an MFMA conv has an int8 "shadow", channel-blocked
    [C_pad16/16][N·H·W][16]: written directly by the producing fused conv block's epilogue, or by
    a shadow node right before the first conv that reads it.

Nodes: one per ExecGroup (build_module.exec_groups) — a fused conv/dense layer
block or residual (qnn.add → clip) block writes all of its ops' outputs (each a
separate trace record) from one kernel.  The node list is built by relay/node_builder.py (one
lowering function per op, looked up in a table); this module allocates the buffers it points into
and holds everything that runs, tunes, replays and measures the built module.
"""
from __future__ import annotations

import atexit
import ctypes
import sys
import weakref
from typing import Callable, Dict, List

import numpy as np

from .. import _lib
from .build_module import Plan, PlanOp, exec_groups
from .node_builder import NodeBuilder, transpose_attrs


def _torch():
    import torch
    return torch


def torch_dtype(name: str):
    torch = _torch()
    return {"int8": torch.int8, "uint8": torch.uint8, "int16": torch.int16, "int32": torch.int32,
            "int64": torch.int64, "float32": torch.float32}[name]


# Every DeviceModule whose native module is alive.  The atexit hook closes them before the
# interpreter finalises (atexit runs first, LIFO after torch's own hooks were registered at import),
# so no tk_module_destroy -- HIP graph / event / stream / hipFree calls -- ever runs from a finaliser
# or after the HIP runtime's static destructors (the round-4 exit SIGSEGV under rocprofv3 was raised
# inside __cxa_finalize).
_LIVE: "weakref.WeakSet[DeviceModule]" = weakref.WeakSet()


@atexit.register
def close_all() -> None:
    """Close every live DeviceModule (also callable directly, e.g. before os._exit)."""
    for m in list(_LIVE):
        try:
            m.close()
        except Exception as e:  # report, keep closing the others
            sys.stderr.write(f"[tachikoma] closing a module at exit failed: {e}\n")


def tune_table_digest(entries) -> str:
    """Digest of a find-step choice: sorted (records, algo) pairs (entries of ``tuning`` or of a
    tune table)."""
    import hashlib
    import json
    return hashlib.sha256(json.dumps(sorted((list(e["records"]), int(e["algo"])) for e in entries)).encode()
                          ).hexdigest()[:16]


class DeviceModule:
    def __init__(self, plan: Plan, params: Dict[str, np.ndarray], dev=None, fuse: bool = True, tune=True):
        """``tune``: True runs the find step (tk_module_tune) on this GPU, False keeps the library's
        own kernel choice, a tune table (``tuning_table()`` output, or the path of its JSON file)
        replays a saved find step so that a profile and a timed run use the same kernels."""
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.TachikomaError("no MI355X visible: the engine runs on the GPU only (no CPU fallback)")
        self.lib = _lib.load()
        self.plan = plan
        self.device = torch.device("cuda", 0) if dev is None else _as_torch_device(dev)
        self.buffers: Dict[str, "torch.Tensor"] = {}
        self._keep: List[object] = []
        self.node_records: List[List[str]] = []  # tk node index -> record names of its outputs
        self.node_kinds: List[str] = []
        self.node_native_kinds: List[int] = []  # tk_node kind (TK_NODE_*) of each node
        # per node: the buffers it reads and writes, by name (relay/replay.py: the plain data the
        # replay schedule is computed from); shadows are "shadow:<tensor>", scratch "<op>:<what>"
        self.node_io: List[dict] = []
        # shadow name -> (TensorRef of its source as the kernels see it, the shadow's buffer)
        self.shadow_sources: Dict[str, tuple] = {}
        # param name -> re-derivations of the build-time buffers computed from it (packed MFMA
        # weights + weight sums), re-run whenever the param's device copy is rewritten
        self._derived: Dict[str, List[Callable[[int], None]]] = {}
        self.groups = exec_groups(plan, fuse=fuse)
        self.tuning: List[dict] = []
        self.tables: Dict[str, object] = {}  # qnn unary ops: op name -> its device lookup table
        # runs as one replayed HIP graph (tk_module_run_graph) instead of host-issued nodes and
        # copies; GraphModule.pick_run_mode chooses by timing both on this host
        self.use_graph = False
        with torch.cuda.device(self.device):
            self._alloc(params)
            self._create(NodeBuilder(self).build())
            if isinstance(tune, (str, dict)):
                self.apply_tuning(tune)
            elif tune:
                self.tune()

    # ------------------------------------------------------------ setup
    def _alloc(self, params):
        torch = _torch()
        for t in self.plan.inputs:
            self.buffers[t.name] = torch.zeros(t.shape, dtype=torch_dtype(t.dtype), device=self.device)
        for t in self.plan.params:
            self.buffers[t.name] = torch.from_numpy(np.ascontiguousarray(params[t.name])).to(self.device)
        for op in self.plan.ops:
            self.buffers[op.name] = torch.empty(op.out.shape, dtype=torch_dtype(op.out.dtype), device=self.device)
        self._alloc_layouts()

    # NHWC data / HWIO, OHWI, HWOI kernels of qnn.conv2d (convolution.cc:718-722): the NCHW / OIHW
    # kernels run between device transposes into untraced buffers named "<op>:nchw_in",
    # "<op>:oihw_w" (re-derived from the param whenever it is rewritten) and "<op>:nchw_out"; the
    # record itself stays in the op's own layout.
    def _alloc_layouts(self):
        self.layout: Dict[str, Dict[str, object]] = {}
        for op in self.plan.ops:
            if op.op == "qnn.conv2d_transpose":
                # runs on NCHW data and an IOHW weight: any other kernel layout goes through "<op>:iohw_w"
                dl, kl = op.attrs["data_layout"], op.attrs["kernel_layout"]
                L = self._alloc_layout(op, dl, kl, "IOHW")
                if dl != "NCHW" or kl != "IOHW":
                    self.layout[op.name] = L
                continue
            if op.op != "qnn.conv2d":
                continue
            dl, kl = op.attrs.get("data_layout", "NCHW"), op.attrs.get("kernel_layout", "OIHW")
            mult = op.attrs.get("depthwise_multiplier", 1)
            if dl == "NCHW" and kl == "OIHW" and mult == 1:
                continue
            ws = tuple(self.plan.tensor(op.inputs[1]).shape[kl.index(ch)] for ch in "OIHW")
            L = self._alloc_layout(op, dl, kl, "OIHW")
            # the grouped-conv weight the kernels read: a depthwise-multiplier weight (C, M, KH, KW)
            # is the same bytes as (C * M, 1, KH, KW) (out channel c * M + m reads [c, m])
            L["w_shape"] = (ws[0] * ws[1], 1, ws[2], ws[3]) if mult > 1 else ws
            self.layout[op.name] = L

    def _alloc_layout(self, op: PlanOp, dl: str, kl: str, kernel: str) -> Dict[str, object]:
        """The buffers ``op``'s NCHW kernel reads and writes: its own, or for NHWC data "<op>:nchw_in"
        and an int32 "<op>:nchw_out", and for a weight not laid out as ``kernel`` its transpose."""
        torch = _torch()
        L: Dict[str, object] = {"x": op.inputs[0], "w": op.inputs[1], "y": op.name}
        if dl == "NHWC":
            xt = self.plan.tensor(op.inputs[0])
            n_, h_, w_, c_ = xt.shape
            L["x"] = f"{op.name}:nchw_in"
            self.buffers[L["x"]] = torch.empty((n_, c_, h_, w_), dtype=torch_dtype(xt.dtype), device=self.device)
            n_, oh, ow, o_ = op.out.shape
            L["y"] = f"{op.name}:nchw_out"
            self.buffers[L["y"]] = torch.empty((n_, o_, oh, ow), dtype=torch.int32, device=self.device)
        if kl != kernel:
            wt = self.plan.tensor(op.inputs[1])
            perm = tuple(kl.index(ch) for ch in kernel)
            L["w"] = f"{op.name}:{kernel.lower()}_w"
            self.buffers[L["w"]] = torch.empty(tuple(wt.shape[k] for k in perm), dtype=torch_dtype(wt.dtype),
                                               device=self.device)
            self._register_transpose(op.inputs[1], L["w"], perm)
        return L

    def _register_transpose(self, src: str, dst: str, perm) -> None:
        """dst = transpose(src) now, and again whenever the param ``src`` is rewritten."""
        x, y = self._ref(src), self._ref(dst)
        ta = transpose_attrs(perm)
        self._keep.append(ta)

        def run(s: int) -> None:
            _lib.check(self.lib.tk_transpose(x.ptr, y.ptr, ctypes.byref(ta), ctypes.c_void_p(s)), f"transpose {src}")
        run(_lib.stream_handle())
        self._derived.setdefault(src, []).append(run)

    def _ref(self, name: str) -> _lib.TensorRef:
        r = _lib.TensorRef.from_torch(self.buffers[name])
        self._keep.append(r)
        return r

    def _scratch(self, nbytes: int, zero: bool = False):
        torch = _torch()
        alloc = torch.zeros if zero else torch.empty
        t = alloc(max(int(nbytes), 16), dtype=torch.uint8, device=self.device)
        self._keep.append(t)
        return t

    def _create(self, nodes: List[_lib.tk_node]) -> None:
        """The native module of ``nodes``, once the packs and transposes queued while building are done."""
        _torch().cuda.current_stream().synchronize()
        self._node_kind_codes = [int(n.kind) for n in nodes]
        self._nodes = nodes  # (their tensors and attrs describe a node's kernels: algo_info)
        arr = (_lib.tk_node * max(1, len(nodes)))(*nodes)
        handle = ctypes.c_void_p()
        _lib.check(self.lib.tk_module_create(arr, len(nodes), ctypes.byref(handle)), "tk_module_create")
        self.handle = handle
        _LIVE.add(self)
        self.n_nodes = len(nodes)

    @property
    def closed(self) -> bool:
        h = getattr(self, "handle", None)
        return h is None or not h.value

    def close(self) -> None:
        """Release the native module (tk_module_destroy: its HIP graphs, events, streams and packed
        capture mirrors) after the device has finished every stream that may still use them, and
        drop the HBM buffers.  Idempotent.  Runs while the HIP runtime is alive: explicitly, from
        the atexit hook below (before interpreter finalisation and before any library's static
        destructors), or from ``__del__`` outside finalisation -- never from a finaliser at process
        teardown, where the runtime (or a profiler's interception tables) may already be gone."""
        h = getattr(self, "handle", None)
        if h is None or not h.value:
            return
        torch = _torch()
        try:
            torch.cuda.synchronize(self.device)
        finally:
            self.handle = None
            _LIVE.discard(self)
            self._destroy_stats_plans()  # their job tables point into the record buffers
            _lib.check(self.lib.tk_module_destroy(h), "tk_module_destroy")
            self.buffers = {}
            self._keep = []

    def __del__(self):
        if sys.is_finalizing():
            return  # leaked on purpose: the process is ending, no HIP calls from finalisers
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ execution
    def _check_value(self, name: str, value):
        """(host array or device tensor) of ``value`` for buffer ``name``; raises on a shape
        mismatch before anything is written."""
        torch = _torch()
        if name not in self.buffers:
            raise KeyError(f"set_input: {name} is not an input or param of the graph")
        buf = self.buffers[name]
        if isinstance(value, torch.Tensor):
            # held to the exact shape, like host arrays (a transposed or NHWC tensor of the same
            # element count must not be reinterpreted silently)
            if tuple(value.shape) != tuple(buf.shape):
                raise ValueError(f"set_input {name}: shape {tuple(value.shape)} vs {tuple(buf.shape)}")
            return value
        v = np.asarray(value.numpy() if hasattr(value, "numpy") else value)
        if tuple(v.shape) != tuple(buf.shape):
            raise ValueError(f"set_input {name}: shape {v.shape} vs {tuple(buf.shape)}")
        return v

    def set_input(self, name: str, value) -> None:
        """GraphExecutor::SetInput (graph_executor.cc:158-166): copy into the module's buffer on
        the current stream, after the last traced run's copies have read it; a param feeding a
        packed MFMA weight is re-packed."""
        self._write(name, self._check_value(name, value))
        self._rederive([name])

    def set_inputs(self, values: Dict[str, object]) -> None:
        """Several buffers at once, every shape checked before the first write."""
        checked = {k: self._check_value(k, v) for k, v in values.items()}
        for k, v in checked.items():
            self._write(k, v)
        self._rederive(list(checked))

    def _write(self, name: str, v) -> None:
        torch = _torch()
        buf = self.buffers[name]
        s = torch.cuda.current_stream(self.device)
        self.wait_capture(s)
        if isinstance(v, torch.Tensor):
            buf.copy_(v.to(buf.dtype).reshape(buf.shape), non_blocking=True)
        else:
            buf.copy_(torch.from_numpy(np.ascontiguousarray(v.astype(np.dtype(str(buf.dtype).replace("torch.", ""))))))

    def _rederive(self, names: List[str]) -> None:
        s = _lib.stream_handle(_torch().cuda.current_stream(self.device))
        for name in names:
            for fn in self._derived.get(name, []):
                fn(s)

    def wait_capture(self, stream=None) -> None:
        """Make ``stream`` wait for the last traced run's D2H copies (tk_module_wait_capture)."""
        _lib.check(self.lib.tk_module_wait_capture(self.handle, ctypes.c_void_p(_lib.stream_handle(stream))),
                   "tk_module_wait_capture")

    def host_dst_array(self, record_ptrs: Dict[str, int]):
        """Per node × output slot host pointers for tk_module_run (NULL = not captured)."""
        slots = self.n_nodes * _lib.MAX_NODE_OUTPUTS
        arr = (ctypes.c_void_p * slots)()
        for i, recs in enumerate(self.node_records):
            for k, name in enumerate(recs):
                if name in record_ptrs:
                    arr[i * _lib.MAX_NODE_OUTPUTS + k] = record_ptrs[name]
        return arr

    def run(self, stream=None, capture_stream=None, host_dst=None) -> None:
        """One run of every node on ``stream`` (+ the record copies on ``capture_stream`` into
        ``host_dst``).  With ``use_graph`` the run is one replayed HIP graph
        (tk_module_run_graph): the copies then execute inside the launch on ``stream``."""
        s = _lib.stream_handle(stream)
        fn = self.lib.tk_module_run_graph if self.use_graph else self.lib.tk_module_run
        what = "tk_module_run_graph" if self.use_graph else "tk_module_run"
        if host_dst is not None:
            _lib.check(fn(self.handle, ctypes.c_void_p(s), ctypes.c_void_p(_lib.stream_handle(capture_stream)),
                          host_dst), what)
        else:
            _lib.check(fn(self.handle, ctypes.c_void_p(s), None, None), what)

    def run_range(self, begin: int, end: int, stream=None) -> None:
        """Nodes [begin, end) only, on ``stream`` (tk_module_run_range; no capture)."""
        _lib.check(self.lib.tk_module_run_range(self.handle, int(begin), int(end),
                                                ctypes.c_void_p(_lib.stream_handle(stream))), "tk_module_run_range")

    def run_order(self, order, stream=None) -> None:
        """The nodes ``order`` in that order, on ``stream`` (tk_module_run_order; no capture)."""
        arr = (ctypes.c_int32 * max(1, len(order)))(*[int(i) for i in order])
        _lib.check(self.lib.tk_module_run_order(self.handle, arr, len(order),
                                                ctypes.c_void_p(_lib.stream_handle(stream))), "tk_module_run_order")

    def replay_plan(self):
        """(node order of a replay, names of the shadows to rebuild up front): relay/replay.py on
        this module's ``node_io``, computed once."""
        if getattr(self, "_replay_plan", None) is None:
            from .replay import replay_order
            self._replay_plan = replay_order(self.node_io, [t.name for t in self.plan.inputs])
        return self._replay_plan

    def rebuild_shadows(self, names=None, stream=None) -> int:
        """Rebuild the shadows ``names`` (default: every shadow whose source is a record or a graph
        input) from their sources as they stand, in one launch (tk_conv2d_make_shadow_batch).
        Returns how many were rebuilt."""
        names = self.replay_plan()[1] if names is None else list(names)
        key = tuple(names)
        cached = getattr(self, "_shadow_batch", None)
        if cached is None or cached[0] != key:
            n = len(names)
            data = (ctypes.POINTER(_lib.tk_tensor) * max(1, n))(*[self.shadow_sources[s][0].ptr for s in names])
            dst = (ctypes.c_void_p * max(1, n))(*[self.shadow_sources[s][1].data_ptr() for s in names])
            self._shadow_batch = cached = (key, data, dst)
        _lib.check(self.lib.tk_conv2d_make_shadow_batch(cached[1], cached[2], len(names),
                                                        ctypes.c_void_p(_lib.stream_handle(stream))),
                   "tk_conv2d_make_shadow_batch")
        return len(names)

    def chain_ops(self) -> List[str]:
        """The records of the tail ops the chain check judges, in report order (node order, then
        chain order): every record of a conv, dense or add block but its first
        (tk_module_chain_ops), computed once."""
        if getattr(self, "_chain_ops", None) is None:
            n = self.lib.tk_module_chain_ops(self.handle, None, 0)
            _lib.check(min(n, 0), "tk_module_chain_ops")
            ops = (_lib.tk_chain_op * max(1, n))()
            _lib.check(min(self.lib.tk_module_chain_ops(self.handle, ops, n), 0), "tk_module_chain_ops")
            self._chain_ops = [self.node_records[ops[k].node][ops[k].output] for k in range(n)]
            self._chain_report = (_lib.tk_wire_mismatch * max(1, n))()
        return self._chain_ops

    def check_chains(self, stream=None) -> Dict[str, tuple]:
        """The chain check on the record buffers as they stand (tk_module_check_chains; after
        load_trace they hold a file's records): {tail record: (count, first flat index)} -- how many
        elements of the record are not its op of its own recorded input, and the first of them
        (_lib.NO_MISMATCH if none).  One launch; returns when it has completed on ``stream``."""
        names = self.chain_ops()
        n = self.lib.tk_module_check_chains(self.handle, self._chain_report, len(names),
                                            ctypes.c_void_p(_lib.stream_handle(stream)))
        _lib.check(min(n, 0), "tk_module_check_chains")
        return {name: (int(r.mismatches), int(r.first)) for name, r in zip(names, self._chain_report)}

    def run_profiled(self, stream=None) -> Dict[str, float]:
        ms = (ctypes.c_float * self.n_nodes)()
        _lib.check(self.lib.tk_module_run_profiled(self.handle, ctypes.c_void_p(_lib.stream_handle(stream)), ms),
                   "tk_module_run_profiled")
        out = {}
        for i, recs in enumerate(self.node_records):
            key = "+".join(recs) if recs else f"<shadow:{i}>"
            out[key] = float(ms[i])
        return out

    def tune(self, max_candidates: int = 16, reps: int = 5, stream=None) -> List[dict]:
        """Find step (tk_module_tune): every MFMA conv-block node keeps the fastest of its first
        ``max_candidates`` kernels, timed on this GPU.  All kernels give bit-identical records.
        Returns (and keeps in ``self.tuning``) per tuned node: records, chosen algo, its time and
        every candidate's."""
        w = max_candidates + 1
        algos = (ctypes.c_int32 * (self.n_nodes * w))()
        us = (ctypes.c_float * (self.n_nodes * w))()
        _lib.check(self.lib.tk_module_tune(self.handle, ctypes.c_void_p(_lib.stream_handle(stream)), max_candidates, reps,
                                           algos, us), "tk_module_tune")
        out = []
        for i in range(self.n_nodes):
            if algos[i * w] < 0:
                continue
            cands = [(int(algos[i * w + 1 + c]), round(float(us[i * w + 1 + c]), 2)) for c in range(max_candidates)
                     if algos[i * w + 1 + c] >= 0]
            out.append({"node": i, "records": list(self.node_records[i]), "algo": int(algos[i * w]),
                        "us": round(float(us[i * w]), 2), "kernel": self.algo_info(i, int(algos[i * w])),
                        "candidates": cands})
        self.tuning = out
        self.tune_table_digest = tune_table_digest(out)
        return out

    def tuning_table(self) -> dict:
        """The find step's choice per conv-block node, keyed by the node's records (stable across
        processes for one plan), with the library it was measured with."""
        return {"format": "tachikoma-tune-table", "version": 2, "library": _lib.build_info(),
                "entries": [{"records": t["records"], "algo": t["algo"], "us": t["us"],
                             "kernel": t.get("kernel") or self.algo_info(t["node"], t["algo"])} for t in self.tuning]}

    def apply_tuning(self, table) -> List[dict]:
        """Replays a tune table (``tuning_table()``, or a JSON file of one) with tk_module_set_node_algo;
        every conv-block node must be listed.  Returns (and keeps in ``self.tuning``) the applied
        entries; the table's digest is ``self.tune_table_digest``."""
        import json
        if isinstance(table, str):
            with open(table) as f:
                table = json.load(f)
        if table.get("format") != "tachikoma-tune-table":
            raise _lib.TachikomaError("not a tachikoma tune table")
        by_records = {tuple(e["records"]): e for e in table["entries"]}
        same_lib = table.get("library") == _lib.build_info()
        applied = []
        for i, (kind, recs) in enumerate(zip(self.node_kinds, self.node_records)):
            if self._node_kind(i) != _lib.NODE_KINDS["conv_block"]:  # dense blocks run as 1x1 conv blocks
                continue
            e = by_records.get(tuple(recs))
            if e is None:
                raise _lib.TachikomaError(f"tune table has no entry for the conv block writing {recs}")
            # algo numbers are plan indices that move when the planner changes: a table from another
            # library is replayed by kernel description (version 2 tables), never by number
            algo = int(e["algo"])
            if algo == 0:
                pass  # the library's own choice (blocks with no kernel list, e.g. depthwise): no description to match
            elif e.get("kernel"):
                if not (same_lib and self.algo_info(i, algo) == e["kernel"]):
                    match = [a for a in self.node_algos(i) if self.algo_info(i, a) == e["kernel"]]
                    if not match:
                        raise _lib.TachikomaError(f"tune table: no kernel '{e['kernel']}' for the conv block "
                                                  f"writing {recs} in this library")
                    algo = match[0]
            elif not same_lib:
                raise _lib.TachikomaError(f"tune table from library {table.get('library')} (this is "
                                          f"{_lib.build_info()}) has no kernel descriptions: algo numbers would "
                                          f"select other kernels")
            _lib.check(self.lib.tk_module_set_node_algo(self.handle, i, algo), "tk_module_set_node_algo")
            applied.append({"node": i, "records": list(recs), "algo": algo, "us": e.get("us"),
                            "kernel": self.algo_info(i, algo), "candidates": []})
        self.tuning = applied
        self.tune_table_digest = tune_table_digest(applied)
        return applied

    def node_algos(self, node: int) -> List[int]:
        """tk_conv2d_block_algos: every kernel (algo) conv-block node `node` can run on."""
        n = self._nodes[node]
        buf = (ctypes.c_int32 * 512)()
        cnt = self.lib.tk_conv2d_block_algos(n.inputs[0], n.inputs[1], ctypes.byref(n.attrs.block), buf, 512)
        _lib.check(min(cnt, 0), "tk_conv2d_block_algos")
        return list(buf[:min(cnt, 512)])

    def algo_info(self, node: int, algo: int) -> str:
        """tk_conv2d_block_algo_info: what kernel `algo` is on conv-block node `node`."""
        n = self._nodes[node]
        buf = ctypes.create_string_buffer(256)
        rc = self.lib.tk_conv2d_block_algo_info(n.inputs[0], n.inputs[1], ctypes.byref(n.attrs.block), int(algo), buf,
                                               len(buf))
        return buf.value.decode() if rc == 0 else f"algo {algo} (not listed)"

    def _node_kind(self, i: int) -> int:
        return self._node_kind_codes[i]

    def set_copy_trace(self, enable: bool) -> None:
        """Per-chunk copy timing of packed traced runs (tk_module_set_copy_trace)."""
        _lib.check(self.lib.tk_module_set_copy_trace(self.handle, int(enable)), "tk_module_set_copy_trace")

    def copy_trace(self) -> List[dict]:
        """The last packed traced run's chunk copies: bytes, start / end ms after the run's first
        launch (tk_module_copy_trace; waits for those copies)."""
        n = self.lib.tk_module_copy_trace(self.handle, None, 0)
        _lib.check(min(n, 0), "tk_module_copy_trace")
        buf = (ctypes.c_double * max(1, 3 * n))()
        _lib.check(min(self.lib.tk_module_copy_trace(self.handle, buf, n), 0), "tk_module_copy_trace")
        return [{"bytes": int(buf[3 * c]), "start_ms": buf[3 * c + 1], "end_ms": buf[3 * c + 2]} for c in range(n)]

    def set_trace_wire(self, enable: bool) -> None:
        """Trace wire of the packed capture: int32 records cross the link narrowed and are widened
        on the host, clip records cross as clamps of the record before them and are rebuilt there
        (tk_module_set_trace_wire; on by default, TK_TRACE_WIRE=0 forces it off, TK_WIRE_CLAMP=0
        at module creation keeps the clip records raw, TK_WIRE_BIAS=0 the bias_add records plain
        differences from their convolution)."""
        _lib.check(self.lib.tk_module_set_trace_wire(self.handle, int(enable)), "tk_module_set_trace_wire")

    def wire_stats(self) -> List[dict]:
        """Per chunk of the last wire run: bytes that crossed the link, raw bytes of the coded
        records, host decode ms (tk_module_wire_stats; waits for the decodes).  Empty when the last
        traced run was not a wire run."""
        n = self.lib.tk_module_wire_stats(self.handle, None, 0)
        _lib.check(min(n, 0), "tk_module_wire_stats")
        buf = (ctypes.c_double * max(1, 3 * n))()
        _lib.check(min(self.lib.tk_module_wire_stats(self.handle, buf, n), 0), "tk_module_wire_stats")
        return [{"wire_bytes": int(buf[3 * c]), "coded_raw_bytes": int(buf[3 * c + 1]), "decode_ms": buf[3 * c + 2]}
                for c in range(n)]

    def set_profiling(self, enable: bool) -> None:
        _lib.check(self.lib.tk_module_set_profiling(self.handle, int(enable)), "tk_module_set_profiling")

    def node_times(self) -> List[float]:
        ms = (ctypes.c_float * self.n_nodes)()
        _lib.check(self.lib.tk_module_node_times(self.handle, ms), "tk_module_node_times")
        return [float(v) for v in ms]

    def records_digest(self, stream=None):
        """Device digest of every trace record (trace_format.records_digest twin), enqueued on
        ``stream``; returns a 1-element int64 device tensor (the u64 digest's bit pattern)."""
        torch = _torch()
        recs = self.plan.records
        if getattr(self, "_digest_slots", None) is None:
            self._digest_slots = torch.zeros(max(1, len(recs)), dtype=torch.int64, device=self.device)
            self._digest_out = torch.zeros(1, dtype=torch.int64, device=self.device)
        s = ctypes.c_void_p(_lib.stream_handle(stream))
        base = self._digest_slots.data_ptr()
        for i, t in enumerate(recs):
            buf = self.buffers[t.name]
            _lib.check(self.lib.tk_digest_bytes(ctypes.c_void_p(buf.data_ptr()), buf.numel() * buf.element_size(),
                                                ctypes.c_void_p(base + 8 * i), s), f"digest {t.name}")
        _lib.check(self.lib.tk_digest_bytes(ctypes.c_void_p(base), 8 * len(recs),
                                            ctypes.c_void_p(self._digest_out.data_ptr()), s), "digest")
        return self._digest_out

    def stats_plan(self, names=None) -> "StatsPlan":
        """The statistics plan (tk_stats_plan) over the record buffers ``names`` (default: every
        record of plan.records, in trace order), built once per name tuple and kept until close().
        Records whose dtype the kernel does not cover are left out and listed in ``skipped``."""
        from ..trace_format import STATS_KIND
        recs = {t.name: t for t in self.plan.records}
        key = tuple(recs) if names is None else tuple(names)
        plans = self.__dict__.setdefault("_stats_plans", {})
        if key not in plans:
            for name in key:
                if name not in recs:
                    raise KeyError(f"stats_plan: {name} is not a record of the graph")
            taken = [n for n in key if str(recs[n].dtype) in STATS_KIND]
            skipped = [n for n in key if str(recs[n].dtype) not in STATS_KIND]
            handle = ctypes.c_void_p()
            if taken:
                n = len(taken)
                src = (ctypes.c_void_p * n)(*[self.buffers[k].data_ptr() for k in taken])
                counts = (ctypes.c_int64 * n)(*[self.buffers[k].numel() for k in taken])
                kinds = (ctypes.c_int32 * n)(*[STATS_KIND[str(recs[k].dtype)] for k in taken])
                _lib.check(self.lib.tk_stats_plan_create(src, counts, kinds, n, ctypes.byref(handle)),
                           "tk_stats_plan_create")
            plans[key] = StatsPlan(handle, taken, [str(recs[k].dtype) for k in taken], skipped)
        return plans[key]

    def _destroy_stats_plans(self) -> None:
        for p in self.__dict__.pop("_stats_plans", {}).values():
            if p.handle:
                self.lib.tk_stats_plan_destroy(p.handle)
                p.handle = ctypes.c_void_p()
        for p in self.__dict__.pop("_fstats_plans", {}).values():
            if p.handle:
                self.lib.tk_fstats_plan_destroy(p.handle)
                p.handle = ctypes.c_void_p()

    def float_stats_plan(self, names=None) -> "FloatStatsPlan":
        """The float statistics plan (tk_fstats_plan) over the float32 record buffers ``names``
        (default: every float32 record of plan.records, in trace order), built once per name tuple
        and kept until close().  A name that is no record is a KeyError, a record that is not
        float32 a ValueError."""
        recs = {t.name: t for t in self.plan.records}
        key = (tuple(n for n, t in recs.items() if str(t.dtype) == "float32") if names is None else tuple(names))
        plans = self.__dict__.setdefault("_fstats_plans", {})
        if key not in plans:
            for name in key:
                if name not in recs:
                    raise KeyError(f"float_stats_plan: {name} is not a record of the graph")
                if str(recs[name].dtype) != "float32":
                    raise ValueError(f"float_stats_plan: record {name} is {recs[name].dtype}, not float32")
            handle = ctypes.c_void_p()
            if key:
                n = len(key)
                src = (ctypes.c_void_p * n)(*[self.buffers[k].data_ptr() for k in key])
                counts = (ctypes.c_int64 * n)(*[self.buffers[k].numel() for k in key])
                _lib.check(self.lib.tk_fstats_plan_create(src, counts, n, ctypes.byref(handle)),
                           "tk_fstats_plan_create")
            plans[key] = FloatStatsPlan(handle, key)
        return plans[key]

    def output(self, name: str):
        return self.buffers[name]


class FloatStatsPlan:
    """A native float statistics plan and the ``names`` of the float32 records it reduces, in the
    order of the result arrays' entries."""

    def __init__(self, handle, names):
        self.handle, self.names = handle, list(names)


class StatsPlan:
    """A native statistics plan and what it covers: ``names`` / ``dtypes`` of the records it
    reduces, in the order of the stats array's entries, and the ``skipped`` names."""

    def __init__(self, handle, names, dtypes, skipped):
        self.handle, self.names, self.dtypes, self.skipped = handle, list(names), list(dtypes), list(skipped)


def _as_torch_device(dev):
    torch = _torch()
    if isinstance(dev, torch.device):
        return dev
    if isinstance(dev, int):
        return torch.device("cuda", dev)
    if hasattr(dev, "device_id"):
        return torch.device("cuda", int(dev.device_id))
    return torch.device(dev)
