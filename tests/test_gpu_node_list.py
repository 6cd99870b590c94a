"""The node list DeviceModule builds, pinned for the three paths that emit more than one node per
group: a layout conv (transposes and a shadow around the NCHW kernel), a dense block that runs as
a 1x1 conv block behind its own shadow node, and a BYOC composite (contraction, then postops).
The expected lists are literals recorded from the builder as it stood before node_builder.py
existed; each graph also runs once and every record is compared with the oracle."""
import numpy as np
import pytest

from oracle import graph_ref
from tachikoma_amd import _lib, relay
from tachikoma_amd.contrib import graph_executor
from tachikoma_amd.relay import qnn
from tachikoma_amd.relay.contrib import tachikoma as tkbyoc
from tests.test_tachikoma_byoc import conv_model

pytestmark = pytest.mark.gpu


def _built(mod, params, inputs):
    """The DeviceModule of ``mod`` after one run whose records all equal the oracle's."""
    gm = graph_executor.GraphModule(relay.build(mod, target="mi355x", params=params)["default"]())
    for k, v in inputs.items():
        gm.set_input(k, v)
    gm.run()
    exp = graph_ref.calibrate(mod, params, inputs)
    assert exp
    for name, e in exp.items():
        np.testing.assert_array_equal(gm.get_node_output(name).numpy(), e, err_msg=name)
    return gm.module


def _io(kind, records, reads, writes, shadows=None):
    return {"kind": kind, "records": records, "reads": reads, "writes": writes, "shadows": shadows or {}}


def test_layout_conv_nodes(device):
    rng = np.random.default_rng(5)
    x = rng.integers(-128, 128, (1, 8, 8, 16)).astype(np.int8)
    w = rng.integers(-128, 128, (3, 3, 16, 16)).astype(np.int8)
    e = qnn.op.conv2d(relay.var("x", x.shape, "int8"), relay.var("w", w.shape, "int8"), relay.const(-3, "int32"),
                      relay.const(2, "int32"), relay.const(0.1), relay.const(0.1), kernel_size=(3, 3), channels=16,
                      padding=(1, 1), data_layout="NHWC", kernel_layout="HWIO")
    m = _built(relay.IRModule.from_expr(e), {"w": w}, {"x": x})
    assert m.node_kinds == ["transpose", "shadow", "qnn.conv2d", "transpose"]
    assert m.node_native_kinds == [_lib.NODE_KINDS[k] for k in m.node_kinds]
    assert m.node_records == [[], [], [], ["%0"]]
    assert m.node_io == [
        _io("transpose", [], ["x"], ["%0:nchw_in"]),
        _io("shadow", [], ["%0:nchw_in"], ["shadow:%0:nchw_in"], {"shadow:%0:nchw_in": "%0:nchw_in"}),
        _io("qnn.conv2d", [], ["%0:nchw_in", "shadow:%0:nchw_in"], ["%0:nchw_out"]),
        _io("transpose", ["%0"], ["%0:nchw_out"], ["%0"])]
    assert m.layout["%0"] == {"x": "%0:nchw_in", "w": "%0:oihw_w", "y": "%0:nchw_out", "w_shape": (16, 16, 3, 3)}
    assert list(m.shadow_sources) == ["shadow:%0:nchw_in"]
    assert len(m._derived["w"]) == 2  # the weight transpose, then the pack that reads its result
    assert tuple(m.buffers["%0:oihw_w"].shape) == (16, 16, 3, 3)


def test_dense_block_runs_as_conv_block(device):
    rng = np.random.default_rng(6)
    params = {"w": rng.integers(-128, 128, (16, 64)).astype(np.int8),
              "b": rng.integers(-500, 500, (16,)).astype(np.int32)}
    x = rng.integers(-128, 128, (2, 64)).astype(np.int8)
    d = qnn.op.dense(relay.var("x", x.shape, "int8"), relay.var("w", (16, 64), "int8"), relay.const(-3, "int32"),
                     relay.const(0, "int32"), relay.const(0.05), relay.const(0.01), units=16)
    y = relay.nn.bias_add(d, relay.var("b", (16,), "int32"), axis=1)
    y = qnn.op.requantize(y, relay.const(np.float32(0.0005)), relay.const(0, "int32"), relay.const(0.1),
                          relay.const(5, "int32"), axis=1, out_dtype="int8")
    y = relay.clip(y, 0.0, 127.0)
    m = _built(relay.IRModule.from_expr(y), params, {"x": x})
    assert m.node_kinds == ["shadow", "dense_block"]
    assert m.node_native_kinds == [_lib.NODE_KINDS["shadow"], _lib.NODE_KINDS["conv_block"]]
    assert m.node_records == [[], ["%0", "%1", "%2", "%3"]]
    assert m.node_io == [
        _io("shadow", [], ["x"], ["shadow:%0:in"], {"shadow:%0:in": "x"}),
        _io("dense_block", ["%0", "%1", "%2", "%3"], ["x", "shadow:%0:in"], ["%0", "%1", "%2", "%3"])]
    assert list(m.shadow_sources) == ["shadow:%0:in"]
    assert {k: len(v) for k, v in m._derived.items()} == {"w": 1}


def test_composite_with_sum_nodes(device):
    mod, params, inputs = conv_model("WithSum")
    m = _built(tkbyoc.partition_for_tachikoma(mod, params), params, inputs)
    # the contraction takes the MFMA path: the graph input's shadow is built right before it
    assert m.node_kinds == ["shadow", "tachikoma.qnn.conv2d:contraction", "tachikoma.qnn.conv2d"]
    assert m.node_native_kinds == [_lib.NODE_KINDS[k] for k in ("shadow", "qnn.conv2d", "postops")]
    assert m.node_records == [[], [], ["%0"]]
    assert m.node_io == [
        _io("shadow", [], ["data"], ["shadow:data"], {"shadow:data": "data"}),
        _io("tachikoma.qnn.conv2d:contraction", [], ["data", "shadow:data"], ["%0:acc"]),
        _io("tachikoma.qnn.conv2d", ["%0"], ["%0:acc", "sum_in"], ["%0"])]
    assert list(m.shadow_sources) == ["shadow:data"]
    assert {k: len(v) for k, v in m._derived.items()} == {"weight": 1}
