"""Pinned host-side plans of the conv / dense dispatch (no GPU): the sizes and listings the library
answers from shapes and attrs alone, against tests/golden/conv_plan_pins.json.  The entry points read
no tensor data, so every tensor here has a null data pointer.

Conv cases: every non-dense geometry of block_value_cases and every geometry of rect_cases, ALGO_CASES
of test_gpu_ops, and the 18 layers of tools/bench_block.py at batch 1, 16 and 64.  Each is taken under
four settings -- as given ("given"), with a residual join ("add"), with kernel_zero_point = 2 (the
per-pixel patch sums, "zw2") and with uint8 weights ("u8w") -- and stores, per setting,
  [scratch bytes of a plain conv, scratch bytes of a block, workspace bytes, number of algos,
   the algo list (runs as a-b), SHA-256 over the "algo:info\\n" lines, the first three of those lines]
which pins the im2col tile plan (row tiles, images per tile, wide stages, the split), the order of the
image-tile plans and the gates of the persistent and dense kernels wherever they reach a size or a
listing.  Dense cases: tk_qnn_dense_workspace_bytes of the dense blocks of block_value_cases.

``python -m tests.test_conv_plan_pins`` prints the JSON the current tree produces."""
import ctypes
import hashlib
import json
import os

from tachikoma_amd import _lib
from tests import block_value_cases as bvc
from tests import rect_cases
from tests.test_gpu_ops import ALGO_CASES
from tools import bench_block

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_pins.json")
SETTINGS = ("given", "add", "zw2", "u8w")
BENCH_BATCHES = (1, 16, 64)


def conv_cases():
    """name -> (x_shape, w_shape, dtype, w_dtype, strides, padding, dilation, groups, zw, zw_vec, has_add)"""
    out = {}
    for prefix, geoms in (("values", bvc.GEOMETRIES), ("rect", rect_cases.GEOMETRIES)):
        for g in geoms:
            if g.dense:
                continue
            kw = g.conv_kw
            out[f"{prefix}/{g.name}"] = (g.x_shape, g.w_shape, g.dtype, g.w_dtype, kw["strides"], kw["padding"],
                                         kw["dilation"], g.groups, g.zw, g.zw_vec, g.residual)
    for i, case in enumerate(ALGO_CASES):
        n, c, h, o, k, st, dt, _za, ap = case[:9]
        out[f"algo{i}"] = ((n, c, h, h), (o, c, k, k), dt, "int8", (st, st), (k // 2,) * 4, (1, 1), 1, 0, False,
                           ap is not None)
    for name, c, h, o, k, s, p in bench_block.SHAPES:
        for b in BENCH_BATCHES:
            out[f"bench/{name}/b{b}"] = ((b, c, h, h), (o, c, k, k), "int8", "int8", (s, s), (p,) * 4, (1, 1), 1, 0,
                                         False, name.startswith("res "))
    return out


def dense_cases():
    return {g.name: (g.x_shape, g.w_shape, g.dtype, g.w_dtype) for g in bvc.GEOMETRIES if g.dense}


def _runs(algos):
    """[1, 16, 17, 18, 3] -> "1,16-18,3" (the order is kept)."""
    parts, i = [], 0
    while i < len(algos):
        j = i
        while j + 1 < len(algos) and algos[j + 1] == algos[j] + 1:
            j += 1
        parts.append(str(algos[i]) if j == i else f"{algos[i]}-{algos[j]}")
        i = j + 1
    return ",".join(parts)


def _measure_conv(lib, case, setting):
    x_shape, w_shape, dtype, w_dtype, strides, padding, dilation, groups, zw, zw_vec, has_add = case
    if setting == "u8w":
        w_dtype = "uint8"
    x, w = _lib.TensorRef(0, x_shape, dtype), _lib.TensorRef(0, w_shape, w_dtype)
    a = _lib.tk_block_attrs()
    a.conv.strides[:], a.conv.padding[:], a.conv.dilation[:] = strides, padding, dilation
    a.conv.groups = groups
    a.conv.input_zero_point = 131 if dtype == "uint8" else -3
    a.conv.kernel_zero_point = 2 if setting == "zw2" else zw
    a.conv.kernel_zero_points = 256 if zw_vec else None  # only tested against NULL on the host
    a.requantize.mode, a.requantize.axis = _lib.TK_RQ_AXIS_UPWARD, 1
    a.has_clip, a.clip_min, a.clip_max = 1, 0, 127
    a.has_add = 1 if has_add or setting == "add" else 0
    conv = ctypes.byref(a.conv)
    scratch = [int(lib.tk_conv2d_scratch_bytes(x.ptr, w.ptr, conv, blk)) for blk in (0, 1)]
    workspace = int(lib.tk_qnn_conv2d_workspace_bytes(x.ptr, w.ptr, conv))
    n = int(lib.tk_conv2d_block_algos(x.ptr, w.ptr, ctypes.byref(a), None, 0))
    assert n >= 0, n
    arr = (ctypes.c_int32 * max(n, 1))()
    assert lib.tk_conv2d_block_algos(x.ptr, w.ptr, ctypes.byref(a), arr, n) == n
    algos = [int(v) for v in arr[:n]]
    buf = ctypes.create_string_buffer(512)
    lines = []
    for al in algos:
        _lib.check(lib.tk_conv2d_block_algo_info(x.ptr, w.ptr, ctypes.byref(a), al, buf, len(buf)))
        lines.append(f"{al}:{buf.value.decode()}\n")
    sha = hashlib.sha256("".join(lines).encode()).hexdigest()
    return scratch + [workspace, n, _runs(algos), sha, [ln.rstrip("\n") for ln in lines[:3]]]


def measure():
    lib = _lib.load()
    conv = {name: {s: _measure_conv(lib, case, s) for s in SETTINGS} for name, case in conv_cases().items()}
    dense = {}
    for name, (x_shape, w_shape, dtype, w_dtype) in dense_cases().items():
        x, w = _lib.TensorRef(0, x_shape, dtype), _lib.TensorRef(0, w_shape, w_dtype)
        dense[name] = int(lib.tk_qnn_dense_workspace_bytes(x.ptr, w.ptr))
    return {"conv": conv, "dense": dense}


def dumps(pins) -> str:
    """One line per case."""
    conv = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in pins["conv"].items())
    return '{\n "conv": {\n' + conv + '\n },\n "dense": ' + json.dumps(pins["dense"]) + "\n}"


def test_conv_plan_pins():
    with open(PINS) as f:
        pins = json.load(f)
    got = json.loads(dumps(measure()))
    assert list(got["conv"]) == list(pins["conv"])
    for name, want in pins["conv"].items():
        assert got["conv"][name] == want, name
    assert got["dense"] == pins["dense"]
    # the cases reach what the docstring says they pin: split-K scratch, the patch, listings with and
    # without the persistent (3, 4) and dense (5) kernels, and blocks that list nothing
    given = {k: v["given"] for k, v in got["conv"].items()}
    assert given["bench/3x3 512->512 7/b64"][:2] == [0, 25690112] and given["bench/3x3 512->512 7/b64"][3] == 112
    assert all(v["zw2"][0] > 0 for k, v in got["conv"].items() if given[k][3] > 0)
    heads = {v[4].split(",")[0] for v in given.values()}
    assert {"", "1", "5"} <= heads
    assert any(v[4].endswith(",3-4") for v in given.values()) and any(v[4] == "1" for v in given.values())


if __name__ == "__main__":
    print(dumps(measure()))
