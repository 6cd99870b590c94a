"""relay/node_builder.py without a GPU: the lowering tables hold exactly the ops the if/elif chain
of DeviceModule._build_nodes had, and the pure fillers write the fields it wrote."""
import ctypes

import pytest

from tachikoma_amd import _lib
from tachikoma_amd.relay import node_builder as nb
from tachikoma_amd.relay.qnn import op as qnn_op

CHAIN_OPS = {
    "qnn.conv2d", "qnn.conv2d_transpose", "qnn.dense", "qnn.requantize", "qnn.add", "qnn.subtract", "qnn.mul",
    "qnn.quantize", "qnn.dequantize", "qnn.concatenate",
    "transpose", "qnn.leaky_relu", "qnn.simulated_quantize", "qnn.simulated_dequantize", "qnn.batch_matmul",
    "nn.bias_add", "clip", "nn.relu", "cast",
    "nn.max_pool2d", "nn.avg_pool2d", "nn.global_avg_pool2d", "nn.batch_flatten", "reshape",
    "annotation.stop_fusion", "annotation.cast_hint", "nn.pad", "ewise", "nn.conv2d", "nn.dense",
}


def test_op_table_is_the_chain():
    assert set(nb.LOWERINGS) == CHAIN_OPS | set(qnn_op.UNARY_OPS)
    assert len(set(qnn_op.UNARY_OPS)) > 0 and not CHAIN_OPS & set(qnn_op.UNARY_OPS)
    for name in nb.LOWERINGS:
        assert nb.lowering_for(name) is nb.LOWERINGS[name]
    # arms that shared a node kind share a function
    for group in (("clip", "nn.relu"),
                  ("nn.batch_flatten", "reshape", "annotation.stop_fusion", "annotation.cast_hint"),
                  ("nn.max_pool2d", "nn.avg_pool2d"), ("qnn.quantize", "qnn.dequantize"),
                  ("qnn.simulated_quantize", "qnn.simulated_dequantize"), ("qnn.add", "qnn.subtract", "qnn.mul"),
                  tuple(qnn_op.UNARY_OPS)):
        assert len({nb.LOWERINGS[name] for name in group}) == 1, group


def test_group_table():
    assert set(nb.GROUP_LOWERINGS) == {"conv_block", "dense_block", "add_block", "tachikoma.qnn.conv2d",
                                       "tachikoma.qnn.dense"}
    assert nb.GROUP_LOWERINGS["conv_block"] is nb.GROUP_LOWERINGS["dense_block"]
    assert nb.GROUP_LOWERINGS["tachikoma.qnn.conv2d"] is nb.GROUP_LOWERINGS["tachikoma.qnn.dense"]


def test_unknown_op_message():
    with pytest.raises(_lib.TachikomaError) as e:
        nb.lowering_for("no.such.op")
    assert str(e.value) == "no device lowering for no.such.op"


def _fields(s):
    values = {f[0]: getattr(s, f[0]) for f in s._fields_}
    return {name: (list(v) if isinstance(v, ctypes.Array) else v) for name, v in values.items()}


def test_per_tensor_requantize_filler():
    """The qnn.concatenate arm: mode, axis -1, multiplier, shift, both zero points, no vectors."""
    pl = {"requant": 1, "mode": _lib.TK_RQ_TENSOR_UPWARD, "multiplier": 1518500250, "shift": -3,
          "input_zero_point": -7, "output_zero_point": 11}
    r = _lib.tk_requantize_attrs()
    nb.fill_rq_tensor(r, pl["mode"], pl["multiplier"], pl["shift"], pl["input_zero_point"], pl["output_zero_point"])
    assert _fields(r) == {"mode": _lib.TK_RQ_TENSOR_UPWARD, "axis": -1, "multiplier": 1518500250, "shift": -3,
                          "multipliers": None, "shifts": None, "input_zero_point": -7, "input_zero_points": None,
                          "output_zero_point": 11}


def test_conv_attrs_without_vectors():
    """A 3x3 stride-2 qnn.conv2d with scalar zero points; the same attrs on the structs that share
    fields with tk_conv2d_attrs fill what those have; a float conv has no zero points."""
    a = {"strides": (2, 2), "padding": (1, 1, 1, 1), "dilation": (1, 1), "groups": 1, "input_zero_point": -3,
         "kernel_zero_point": 2, "kernel_size": (3, 3), "channels": 16, "output_padding": (1, 0)}
    ca = _lib.tk_conv2d_attrs()
    nb.conv_attrs(ca, a, {})
    assert _fields(ca) == {"strides": [2, 2], "padding": [1, 1, 1, 1], "dilation": [1, 1], "groups": 1,
                           "input_zero_point": -3, "kernel_zero_point": 2, "kernel_zero_points": None}
    ta = _lib.tk_conv2d_transpose_attrs()
    nb.conv_attrs(ta, a, {})
    assert _fields(ta) == {"strides": [2, 2], "padding": [1, 1, 1, 1], "output_padding": [1, 0], "groups": 1,
                           "input_zero_point": -3, "kernel_zero_point": 2, "kernel_zero_points": None}
    da = _lib.tk_dense_attrs()
    nb.conv_attrs(da, {"input_zero_point": 4, "kernel_zero_point": -1, "units": 8}, {})
    assert _fields(da) == {"input_zero_point": 4, "kernel_zero_point": -1, "kernel_zero_points": None}
    fa = _lib.tk_conv2d_attrs()
    nb.conv_attrs(fa, {k: a[k] for k in ("strides", "padding", "dilation", "groups")}, {})
    assert _fields(fa) == dict(_fields(ca), input_zero_point=0, kernel_zero_point=0)


def test_error_constant():
    assert (_lib.TK_ERR_INVALID_ARG, _lib.TK_ERR_SHAPE, _lib.TK_ERR_FORMAT) == (-1, -3, -7)
