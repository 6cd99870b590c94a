"""Dump every DeviceModule that a run of the GPU module tests builds, in a pointer-free form, one
JSON line per module: `python tools/dump_node_list.py OUT`.  Two trees whose node builders agree
write equal files (compare them byte for byte, or by the digest this prints); constants appear
as dtype, shape and a digest of their bytes, scratch and node-written buffers without a digest."""
import ctypes
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytest  # noqa: E402
import torch  # noqa: E402

from tachikoma_amd import _lib  # noqa: E402
from tachikoma_amd.relay import device_module as dm  # noqa: E402

FILES = ["test_gpu_qnn_ops.py", "test_gpu_module.py", "test_gpu_models.py", "test_gpu_realize.py",
         "test_gpu_requantize_fp.py", "test_tachikoma_byoc.py", "test_gpu_executor_api.py"]
WORDS = ctypes.sizeof(_lib.tk_node_attrs) // 8
seconds = []


def _describe(t, digest):
    d = f"{str(t.dtype)[6:]}{list(t.shape)}"
    if digest:
        d += "#" + hashlib.sha1(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:12]
    return d


def dump(m) -> dict:
    written = {n.outputs[k].contents.data for n in m._nodes for k in range(n.n_outputs)}
    written |= m.__dict__.pop("_scratch_ptrs", set())
    label = {}
    for name, buf in m.buffers.items():
        label.setdefault(buf.data_ptr(), name)
    for t in m._keep:
        if isinstance(t, torch.Tensor):
            label.setdefault(t.data_ptr(), _describe(t, t.data_ptr() not in written))

    def tensor(p):
        t = p.contents
        return [label.get(t.data, "?"), [t.shape[k] for k in range(t.ndim)], [t.dtype.code, t.dtype.bits]]

    nodes = []
    for n in m._nodes:
        words = (ctypes.c_uint64 * WORDS).from_buffer_copy(n.attrs)
        nodes.append({"kind": int(n.kind), "n_inputs": n.n_inputs, "n_outputs": n.n_outputs,
                      "inputs": [tensor(n.inputs[k]) for k in range(n.n_inputs)],
                      "outputs": [tensor(n.outputs[k]) for k in range(n.n_outputs)],
                      "ext": [label.get(e, "?") if e else None for e in n.ext],
                      "attrs": [label.get(w, w) for w in words]})
    return {"nodes": nodes, "native_kinds": m.node_native_kinds, "kind_codes": m._node_kind_codes,
            "node_kinds": m.node_kinds, "node_records": m.node_records, "node_io": m.node_io,
            "shadow_sources": list(m.shadow_sources), "derived": {k: len(v) for k, v in m._derived.items()},
            "layout": {k: {a: list(b) if isinstance(b, tuple) else b for a, b in v.items()}
                       for k, v in m.layout.items()}, "tables": list(m.tables), "n_nodes": m.n_nodes}


def main(out: str) -> int:
    init, scratch = dm.DeviceModule.__init__, dm.DeviceModule._scratch

    def traced_scratch(self, *a, **k):
        t = scratch(self, *a, **k)
        self.__dict__.setdefault("_scratch_ptrs", set()).add(t.data_ptr())
        return t

    def traced_init(self, *a, **k):
        t0 = time.perf_counter()
        init(self, *a, **k)
        seconds.append(time.perf_counter() - t0)
        with open(out, "a") as f:
            f.write(json.dumps(dump(self), sort_keys=True) + "\n")

    dm.DeviceModule._scratch, dm.DeviceModule.__init__ = traced_scratch, traced_init
    open(out, "w").close()
    rc = pytest.main([os.path.join(ROOT, "tests", f) for f in FILES] + ["-q", "-p", "no:cacheprovider"])
    with open(out, "rb") as f:
        data = f.read()
    print(json.dumps({"modules": data.count(b"\n"), "sha256": hashlib.sha256(data).hexdigest(), "pytest_exit": int(rc),
                      "module_creation_s": round(sum(seconds), 3)}))
    return int(rc)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
