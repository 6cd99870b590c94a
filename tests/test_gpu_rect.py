"""The conv, depthwise, pool and add kernels on non-square geometry (tests/rect_cases.py) against
the CPU oracle, bit for bit: rectangular planes, 1x7 / 7x1 / 3x5 kernels, unequal strides,
dilations and paddings, on every kernel the block lists for the case's attrs.  Every other GPU
test of a fused block is square in all of these, so that a kernel which swapped H and W, sh and sw
or the top and left padding would pass it; test_rect_cases.py proves of the reference alone that
such a swap changes the expected records here.
"""
import re

import numpy as np
import pytest

from oracle import graph_ref
from oracle import qnn_ref as ref
from tests import block_value_cases as bvc
from tests import rect_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tk(device):
    from tests import tk_gpu
    return tk_gpu


def _run(tk, c, algo=0, **extra):
    g = c.geom
    kw = dict(clip=g.clip, out_dtype=g.dtype, want_shadow=True, poison=True, rounding=c.rounding, rq_zp=c.rq_zp,
              zw_vec=c.zw_vec, **g.conv_kw)
    if c.residual is not None:
        kw.update(residual=c.residual, add_params=c.add_params, block_is_rhs=g.block_is_rhs)
    return tk.conv2d_block(c.x, c.w, c.bias, g.za, g.zw, c.s_in, bvc.S_OUT, g.zp_out, algo=algo, **kw, **extra)


def _listed(tk, c):
    """(algo, description) of every kernel the block lists for this case's attrs."""
    return _run(tk, c, algos_only=True, algo_info=True)


def _differences(label, got, e):
    """One line on where got differs from e, or none."""
    assert got.shape == e.shape and got.dtype == e.dtype, (label, got.shape, got.dtype, e.shape, e.dtype)
    if np.array_equal(got, e):
        return []
    where = np.argwhere(got != e)
    first = tuple(where[0].tolist())
    return [f"{label}: {len(where)} of {e.size} differ, first at {list(first)} ({got[first]} for {e[first]}), "
            f"index ranges {where.min(0).tolist()}..{where.max(0).tolist()}"]


@pytest.mark.parametrize("name,mode", rc.CASE_IDS, ids=["-".join(i) for i in rc.CASE_IDS])
def test_rect_block(tk, name, mode):
    """Every record and the shadow of the block, on the library's choice (algo 0) and on each
    listed kernel, equal the oracle's."""
    c = rc.build(name, mode)
    exp = c.expected + [c.shadow]
    what = ["conv", "bias_add", "requantize"] + (["add"] if c.residual is not None else []) + ["clip", "shadow"]
    bad = []
    for algo, desc in [(0, "the library's choice")] + _listed(tk, c):
        outs = _run(tk, c, algo=algo)
        assert len(outs) == len(exp)
        for label, got, e in zip(what, outs, exp):
            bad += _differences(f"algo {algo} ({desc}) {label}", got, e)
    assert not bad, "\n".join(bad)


def test_rect_families(tk):
    """The rectangular planes still reach the kernel families of their square twins: im2col tiles
    (1), both persistent algos (3, 4), image-tile plans of 32 and of 64 rows, a split-K image plan,
    3x3 and 1x1 plans.  A geometry with an unequal kernel, stride, dilation or padding lists at
    least algo 1 and no image-tile plan (algos from 16); exactly the depthwise, grouped and tiny-Cin
    geometries list nothing."""
    algos, descs, single = set(), [], []
    for g in rc.GEOMETRIES:
        for mode in rc.MODES:
            listed = _listed(tk, rc.build(g.name, mode))
            print(g.name, mode, listed)
            if g in rc.RECT:
                algos |= {a for a, _ in listed}
                descs += [d for a, d in listed if a >= 16]
            if g in rc.ANISO:
                assert 1 in {a for a, _ in listed} and not [a for a, _ in listed if a >= 16], (g.name, mode, listed)
            if not listed and mode == "AXIS_UPWARD":
                single.append(g.name)
    assert {1, 3, 4} <= algos, sorted(algos)
    img = [d for d in descs if d.startswith("image tiles")]
    assert img, descs[:10]
    heads = [d.split("; split K")[0] for d in img]  # the plan itself, without its split-K epilogue pass
    for pattern in (r": 32 rows x", r": 64 rows x", r"\b3x3\b", r"\b1x1\b"):
        assert any(re.search(pattern, d) for d in heads), (pattern, sorted(set(heads))[:40])
    assert any("; split K" in d for d in img), sorted(set(img))[:40]
    assert sorted(single) == sorted(g.name for g in rc.SINGLE)


@pytest.mark.parametrize("name,zw_vec", [(n, False) for n in rc.PLAIN] + [("k3x5_s21", True)])
def test_rect_conv2d_plain(tk, name, zw_vec):
    """The un-fused tk_qnn_conv2d, with its own tile and split decisions."""
    g = rc.GEOMETRY[name]
    x, w, zv, conv = rc.operands(name)
    if zw_vec:
        zv = bvc._rng("rect", name, "zw_vec").integers(-6, 7, size=g.o).astype(np.int32)
        conv = ref.qnn_conv2d(x, w, g.za, zv, **g.conv_kw)
    got = tk.conv2d(x, w, g.za, g.zw, zw_vec=zv, **g.conv_kw)
    bad = _differences("conv", got, conv)
    assert not bad, bad[0]


@pytest.mark.parametrize("dtype", list(rc.POOL_CASES))
def test_rect_pools(tk, dtype):
    """max and avg pools with unequal windows, strides, paddings and dilations."""
    x = rc.pool_input(dtype)
    bad = []
    for size, strides, padding, dilation in rc.POOL_SETTINGS:
        kw = dict(pool_size=size, strides=strides, padding=padding, dilation=dilation)
        label = f"{size} s{strides} p{padding} d{dilation}"
        bad += _differences(f"max_pool2d {label}", tk.pool("tk_max_pool2d", x, **kw), ref.max_pool2d(x, **kw))
        for include in (False, True):
            bad += _differences(f"avg_pool2d {label} count_include_pad={include}",
                                tk.pool("tk_avg_pool2d", x, count_include_pad=include, **kw),
                                ref.avg_pool2d(x, count_include_pad=include, **kw))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", list(rc.POOL_SHADOW_CASES))
def test_rect_max_pool_shadow(tk, dtype):
    """tk_max_pool2d_shadow with non-square windows: the record and the output shadow."""
    x = rc.pool_input(dtype, rc.POOL_SHADOW_CASES[dtype])
    bad = []
    for size, strides, padding, dilation in rc.POOL_SETTINGS[:2]:
        rec, shadow = tk.max_pool_shadow(x, size, strides, padding, dilation)
        exp = ref.max_pool2d(x, size, strides, padding, dilation)
        bad += _differences(f"{size} record", rec, exp) + _differences(f"{size} shadow", shadow, bvc.blocked_shadow(exp))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", rc.GLOBAL_DTYPES)
def test_rect_global_avg_pool(tk, dtype):
    """tk_global_avg_pool2d on planes of one element past a wave (65), a wave (64), one short (63)
    and 150 elements."""
    bad = []
    for plane in rc.GLOBAL_PLANES:
        x = rc.pool_input(dtype, (2, 5) + plane)
        bad += _differences(f"{plane}", tk.global_avg_pool(x), ref.global_avg_pool2d(x))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape,dtype", [((3, 40, 5, 9), "uint8"), ((2, 64, 4, 14), "int8")])
def test_rect_add_block(tk, shape, dtype):
    """tk_qnn_add_block with clip and shadow on rectangular planes."""
    rng = bvc._rng("rect", "add_block", shape)
    a, b = bvc._uniform(rng, shape, dtype), bvc._uniform(rng, shape, dtype)
    lo, hi = ref.dtype_range(dtype)
    clip = (lo + 40, hi - 30)
    outs = tk.qnn_add_block(a, b, *bvc.ADD_PARAMS[dtype], clip=clip, want_shadow=True)
    add = ref.qnn_add(a, b, *bvc.ADD_PARAMS[dtype])
    clipped = ref.clip(add, *clip)
    assert len(outs) == 3
    bad = _differences("add", outs[0], add) + _differences("clip", outs[1], clipped)
    bad += _differences("shadow", outs[2], bvc.blocked_shadow(clipped))
    assert not bad, "\n".join(bad)


def _rect_model():
    """uint8 (2, 3, 20, 36) -> 3x3 stride-2 stem padded (0, 0, 1, 1) -> depthwise 3x3 -> 1x1 expand
    joined with a 1x1 of the stem -> (3, 2) stride-(2, 1) max pool -> 1x7 -> 7x1 -> global average
    pool -> dense."""
    from tachikoma_amd import relay, zoo
    from tachikoma_amd.relay import qnn
    b = zoo._Builder(7)
    shape = (2, 3, 20, 36)

    def block(x, name, cout, k, stride=(1, 1), pad=(0, 0, 0, 0), groups=1, act="relu"):
        cin = x.expr.shape[1]
        fan = (cin // groups) * k[0] * k[1]
        w = b.weight(f"{name}.weight", (cout, cin // groups) + tuple(k))
        bias = b.bias(f"{name}.bias", cout)
        s_w = b.wscale(cout, fan, x.sigma)
        y = qnn.op.conv2d(x.expr, w, relay.const(x.zp, "int32"), relay.const(0, "int32"),
                          relay.const(x.scale, "float32"), relay.const(s_w, "float32"), kernel_size=tuple(k),
                          channels=cout, strides=stride, padding=pad, groups=groups)
        y = relay.nn.bias_add(y, bias, axis=1)
        s_out = zoo._requant_out_scale(x.scale, s_w, fan, x.sigma)
        zp_out = b.zp()
        y = qnn.op.requantize(y, relay.const((np.float32(x.scale) * s_w).astype(np.float32), "float32"),
                              relay.const(0, "int32"), relay.const(s_out, "float32"), relay.const(zp_out, "int32"),
                              axis=1, out_dtype="int8")
        if act:
            y = relay.clip(y, float(zp_out), 127.0)
        return zoo.QTensor(y, s_out, zp_out, 20.0 if act else 32.0)

    x = zoo.QTensor(relay.var("data", shape=shape, dtype="uint8"), 0.0235, 131, 73.9)
    stem = block(x, "stem", 16, (3, 3), stride=(2, 2), pad=(0, 0, 1, 1))                     # (2, 16, 10, 18)
    y = block(stem, "dw", 16, (3, 3), pad=(1, 1, 1, 1), groups=16)
    y = zoo.qadd(b, block(y, "expand", 64, (1, 1), act=None), block(stem, "side", 64, (1, 1), act=None))
    y = zoo.QTensor(relay.nn.max_pool2d(y.expr, pool_size=(3, 2), strides=(2, 1)), y.scale, y.zp, y.sigma)  # (2, 64, 4, 17)
    y = block(y, "k1x7", 32, (1, 7), pad=(0, 3, 0, 3))
    y = block(y, "k7x1", 32, (7, 1), pad=(3, 0, 3, 0))
    out = zoo._head(b, y, classes=10)
    return zoo.Model("rect_graph", relay.IRModule.from_expr(out.expr), b.params, "data", shape, "uint8", 7)


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
def test_rect_graph_trace(device, tmp_path, fuse):
    """A non-square graph through shape inference, fusion, the node builder's shadow allocation and
    the packed capture: every record of the trace equals the graph oracle's."""
    from tests.test_gpu_models import _compare, _run_trace
    model = _rect_model()
    x = bvc._uniform(bvc._rng("rect", "graph"), model.input_shape, "uint8")
    _, tr = _run_trace(model, x, tmp_path, fuse=fuse)
    exp = graph_ref.calibrate(model.mod, model.params, {"data": x})
    shapes = {tuple(e.shape[2:]) for e in exp.values() if e.ndim == 4}
    assert {(10, 18), (4, 17)} <= shapes, shapes
    assert set(tr.records) == set(exp)
    _compare(tr.records, exp)
