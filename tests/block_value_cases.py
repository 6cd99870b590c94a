"""Shared cases of the fused-block value tests (CPU reference checks in test_block_value_cases.py,
the kernels in test_gpu_block_values.py): a case is a *geometry* (the smallest shape at which one
kernel family is still listed) times a *value regime* times a requantize mode, and carries the
block's inputs, its attrs and every expected record.  All expected records come from
oracle.qnn_ref: qnn_conv2d / qnn_dense -> bias_add -> requantize -> [qnn_add] -> clip, then
blocked_shadow of the last record for the 4-D blocks.

Regimes (s_out = 0.05; sigma_c = per-channel standard deviation of the oracle's own conv record):

  calibrated  uniform 8-bit operands, bias in +-2^14, M[c] = 48 / sigma_c * U[0.5, 2] with every 8th
              channel snapped to a power of two, s_in = float32(M * s_out), input_zero_points a
              vector in [-1000, 1000).  Modes AXIS_UPWARD, AXIS_TONEAREST.
  wrap        as calibrated, but bias[c] within 2^16 of INT32_MAX (c % 4 == 0), of INT32_MIN
              (c % 4 == 1) or uniform over int32, and input_zero_points[c] =
              wrap_i32(bias[c] + U[-1000, 1000)): the bias add wraps and the zero-point subtraction
              wraps back to roughly the conv.  Modes AXIS_UPWARD, AXIS_TONEAREST.
  tensor      operands and bias as calibrated, a scalar scale 48 / sigma * s_out: as it is with the
              scalar input_zero_point 37 (TENSOR_UPWARD), snapped to a power of two with the
              per-axis vector (TENSOR_POW2) and snapped with the scalar 37 under TONEAREST
              (TENSOR_TONEAREST).
  small       data in za + [-2, 2], weights in {-1, 0, 1}, bias in [-30, 30).  AXIS_UPWARD and
              AXIS_TONEAREST: M = geomspace(2^-3, 3, O), every 4th channel snapped to a power of
              two, input_zero_points a vector in [-4, 4) (right shifts below 2 and left shifts: the
              general requantize form on unsaturated data with many exact ties).  TENSOR_POW2 and
              TENSOR_TONEAREST: the scalar 0.25 * s_out with zero point 1.  IDENTITY: s_in
              bit-equal to s_out, zero point 5.

All regimes: uint8 geometries use za = 131 and zp_out = 120, int8 ones zp_out = -3; residual
geometries draw the residual uniformly over the dtype and take the add params of
test_gpu_ops.RESIDUAL_CASES; the clip is (lo + 40, hi - 30), so that both bounds and the values
between them occur.

What the reference alone gives (test_block_value_cases.py asserts the bounds in brackets for every
geometry; these are the minima over all geometries, with the geometry that sets them):

  unsaturated share of the requantize record [>= 0.5]
      calibrated 0.811 (direct_5x5)   wrap 0.897 (direct_5x5)   tensor 0.913 (dw_planes_s2)
      small AXIS 0.935 (split_im2col_256)   small 0.25 scalar 1.0   IDENTITY 0.985 (split_im2col_256)
  distinct byte values, calibrated / wrap [>= 200; a record of fewer than 200 elements: half its
      element count]: 256 in every record but dense_tiles_96 (254 of 3840 elements), direct_5x5
      (234 of 864) and dense_5x84x10 (42 of 50)
  wrap share of the bias add, wrap [>= 0.10]: 0.148 (stage128_1x1_res)
  AXIS_UPWARD vs AXIS_TONEAREST records differing, small [>= 0.01]: 0.015 (direct_5x5)
  UPWARD vs TONEAREST records differing at the 0.25 scalar, small [>= 0.05]: 0.103 (stage128_1x1_res)

Two draws are narrower than their first statement, because a bound was missed with it: in wrap, a
bias sits within min(2^16, sigma_c) of its int32 bound (with 2^16 alone the 9- and 24-term convs
never reach past it: wrap shares of 0.0 to 0.085), and SEED was chosen so that the rounding
conditions also hold in the records of 50 and 864 elements, where few channels are powers of two.
"""
import functools
import zlib
from dataclasses import dataclass, field
from typing import Optional, Tuple, Union

import numpy as np

from oracle import qnn_ref as ref

S_OUT = np.float32(0.05)
MODES = ["IDENTITY", "TENSOR_POW2", "TENSOR_UPWARD", "TENSOR_TONEAREST", "AXIS_UPWARD", "AXIS_TONEAREST"]
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

# add params (lhs s/zp, rhs s/zp, out s/zp) of test_gpu_ops.RESIDUAL_CASES, by dtype
ADD_PARAMS = {"int8": (0.05, 3, 0.07, -2, 0.09, 1), "uint8": (0.1, 130, 0.2, 120, 0.15, 128)}

# (regime, mode): every mode a regime is run under
VARIANTS = [
    ("calibrated", "AXIS_UPWARD"), ("calibrated", "AXIS_TONEAREST"),
    ("wrap", "AXIS_UPWARD"), ("wrap", "AXIS_TONEAREST"),
    ("tensor", "TENSOR_UPWARD"), ("tensor", "TENSOR_POW2"), ("tensor", "TENSOR_TONEAREST"),
    ("small", "AXIS_UPWARD"), ("small", "AXIS_TONEAREST"), ("small", "TENSOR_POW2"), ("small", "TENSOR_TONEAREST"),
    ("small", "IDENTITY"),
]


def _tup(v, n):
    """An attribute given as one value for every axis or side, or as its n values."""
    return (v,) * n if isinstance(v, int) else tuple(v)


@dataclass(frozen=True)
class Geometry:
    name: str
    meant: str                      # the kernel family this shape is here for
    x_shape: Tuple[int, ...]        # NCHW, or [M, K] of a dense block
    o: int
    k: Union[int, Tuple[int, int]] = 1                  # one value for both axes, or (KH, KW)
    stride: Union[int, Tuple[int, int]] = 1             # ... or (sh, sw)
    pad: Union[int, Tuple[int, int, int, int]] = 0      # one value for all sides, or (pt, pl, pb, pr)
    groups: int = 1
    dtype: str = "int8"             # data, residual and output dtype
    zw: int = 0
    zw_vec: bool = False            # per-output-channel kernel zero points
    residual: bool = False
    block_is_rhs: bool = False
    dense: bool = False             # tk_qnn_dense_block instead of tk_qnn_conv2d_block
    dilation: Union[int, Tuple[int, int]] = 1           # one value for both axes, or (dh, dw)
    w_dtype: str = "int8"           # weight dtype

    @property
    def za(self):
        return 131 if self.dtype == "uint8" else -3

    @property
    def zp_out(self):
        return 120 if self.dtype == "uint8" else -3

    @property
    def clip(self):
        lo, hi = ref.dtype_range(self.dtype)
        return lo + 40, hi - 30

    @property
    def w_shape(self):
        if self.dense:
            return self.o, self.x_shape[1]
        return (self.o, self.x_shape[1] // self.groups) + _tup(self.k, 2)

    @property
    def conv_kw(self):
        return dict(strides=_tup(self.stride, 2), padding=_tup(self.pad, 4), dilation=_tup(self.dilation, 2),
                    groups=self.groups)


GEOMETRIES = [
    Geometry("img3x3_64", "3x3 image tiles, 32/64-channel stages, several images per workgroup (last partial)",
             (3, 64, 14, 14), 64, k=3, pad=1),
    Geometry("stage128_1x1", "128-channel stages; persistent algos 3 and 4 under the UPWARD modes",
             (2, 128, 12, 12), 64),
    Geometry("stage128_1x1_res", "as stage128_1x1 with a residual join, the block on the rhs",
             (2, 128, 12, 12), 64, residual=True, block_is_rhs=True),
    Geometry("split_img_160", "split-K image plans", (4, 160, 7, 7), 64, k=3, pad=1),
    Geometry("split_im2col_256", "split-K im2col", (2, 256, 7, 7), 64, k=3, pad=1),
    Geometry("rows128_512", "128-row tiles", (2, 512, 10, 10), 128),
    Geometry("cols256_1024", "256-column tiles (a grid of >= 256 tiles)", (16, 64, 14, 14), 1024),
    Geometry("chunk32_144_u8_res", "partial 32-row chunk, uint8, residual join", (3, 24, 28, 28), 144, dtype="uint8",
             residual=True),
    Geometry("dense_tiles_96", "dense tile kernel (algo 5), kernel zero point 0", (40, 512, 1, 1), 96),
    Geometry("dw_bands", "depthwise row bands", (2, 16, 56, 56), 16, k=3, pad=1, groups=16),
    Geometry("dw_planes_s2", "depthwise whole planes, stride 2", (2, 32, 28, 28), 32, k=3, stride=2, pad=1, groups=32),
    Geometry("dw_flat", "depthwise flat groups", (2, 64, 7, 7), 64, k=3, pad=1, groups=64),
    Geometry("dw_u8_zwvec", "depthwise, uint8 data, per-channel kernel zero points", (2, 32, 14, 14), 32, k=3, pad=1,
             groups=32, dtype="uint8", zw_vec=True),
    Geometry("dw_band_pad3", "depthwise band kernel (padding above 2: the tile kernel declines; 32x32 outputs)",
             (1, 16, 28, 28), 16, k=3, pad=3, groups=16),
    Geometry("direct_5x5", "direct kernel (tiny Cin, O < 16)", (1, 1, 12, 12), 6, k=5, pad=2),
    Geometry("dense_5x84x10", "tk_qnn_dense_block, one ragged tile", (5, 84), 10, dense=True),
    Geometry("dense_130x70x129", "tk_qnn_dense_block, four tiles, uint8 data, kernel zero point 2", (130, 70), 129,
             dtype="uint8", zw=2, dense=True),
]
GEOMETRY = {g.name: g for g in GEOMETRIES}
CASE_IDS = [(g.name, regime, mode) for g in GEOMETRIES for regime, mode in VARIANTS]


@dataclass
class Case:
    geom: Geometry
    regime: str
    mode: str
    x: np.ndarray
    w: np.ndarray
    bias: np.ndarray
    zw_vec: Optional[np.ndarray]
    s_in: np.ndarray                # float32 scalar or per-axis vector
    rq_zp: np.ndarray               # int32 scalar (input_zero_point) or vector (input_zero_points)
    rounding: str
    residual: Optional[np.ndarray]
    add_params: Optional[tuple]
    expected: list = field(default_factory=list)   # records in chain order
    shadow: Optional[np.ndarray] = None            # blocked_shadow of the last record (4-D blocks)

    @property
    def requantize_record(self):
        return self.expected[2]


def blocked_shadow(x: np.ndarray) -> np.ndarray:
    """Expected tk_conv2d_make_shadow layout of an NCHW 8-bit tensor: [C_pad16/16][N*H*W][16] uint8,
    padded channels 0, uint8 stored xor 0x80."""
    n, c, h, w = x.shape
    cpad = (c + 15) // 16 * 16
    b = x.view(np.uint8) ^ (0x80 if x.dtype == np.uint8 else 0)
    full = np.zeros((n, cpad, h, w), np.uint8)
    full[:, :c] = b
    return full.reshape(n, cpad // 16, 16, h * w).transpose(1, 0, 3, 2).reshape(cpad // 16, n * h * w, 16)


SEED = 10  # of every draw; chosen so that the smallest records (50 elements) meet the reference conditions too


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr((SEED,) + key).encode()))  # PYTHONHASHSEED-independent


def _uniform(rng, shape, dtype):
    info = np.iinfo(dtype)
    return rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dtype)


@functools.lru_cache(maxsize=None)
def operands(name: str, small: bool):
    """(x, w, zw_vec, conv record) of a geometry: the uniform 8-bit operands that calibrated, wrap
    and tensor share, or the small ones.  The oracle's conv is computed once per geometry and
    operand kind; the arrays are shared between cases and must not be written to."""
    g = GEOMETRY[name]
    rng = _rng(name, "small" if small else "uniform")
    if small:
        x = (g.za + rng.integers(-2, 3, size=g.x_shape)).astype(g.dtype)
        w = rng.integers(-1, 2, size=g.w_shape).astype(np.int8)
    else:
        x = _uniform(rng, g.x_shape, g.dtype)
        w = _uniform(rng, g.w_shape, g.w_dtype)
    zv = rng.integers(-6, 7, size=g.o).astype(np.int32) if g.zw_vec else None
    zw = zv if zv is not None else g.zw
    conv = ref.qnn_dense(x, w, g.za, zw) if g.dense else ref.qnn_conv2d(x, w, g.za, zw, **g.conv_kw)
    for a in (x, w, zv, conv):
        if a is not None:
            a.setflags(write=False)
    return x, w, zv, conv


def _sigma(conv):
    """Per-channel (axis 1) standard deviation of a conv record, at least 1."""
    per = np.moveaxis(conv, 1, 0).reshape(conv.shape[1], -1).astype(np.float64).std(axis=1)
    return np.maximum(per, 1.0)


def _snap(m):
    return 2.0 ** np.round(np.log2(m))


def _scale(m):
    """s_in = float32(M * s_out); exact for a power-of-two M."""
    return (np.asarray(m, np.float64) * np.float64(S_OUT)).astype(np.float32)


def _draw(g: Geometry, regime: str, mode: str, conv):
    """(bias, s_in, rq_zp) of a case.  Both modes of a regime see the same draws."""
    rng = _rng(g.name, regime)
    o = g.o
    if regime == "small":
        bias = rng.integers(-30, 30, size=o).astype(np.int32)
        m = np.geomspace(2.0 ** -3, 3.0, o)
        m[::4] = _snap(m[::4])
        zp_vec = rng.integers(-4, 4, size=o).astype(np.int32)
        if mode.startswith("AXIS"):
            return bias, _scale(m), zp_vec
        if mode == "IDENTITY":
            return bias, np.float32(S_OUT), np.int32(5)
        return bias, _scale(0.25)[()], np.int32(1)
    bias = rng.integers(-2 ** 14, 2 ** 14, size=o).astype(np.int32)
    sigma = _sigma(conv)
    m = 48.0 / sigma * rng.uniform(0.5, 2.0, size=o)
    m[::8] = _snap(m[::8])
    zp_vec = rng.integers(-1000, 1000, size=o).astype(np.int32)
    if regime == "calibrated":
        return bias, _scale(m), zp_vec
    if regime == "wrap":
        c = np.arange(o)
        # within 2^16 of the bound, and within sigma_c where that is less, so that the conv reaches past it
        near = (rng.uniform(0, 1, size=o) * np.minimum(2.0 ** 16, sigma)).astype(np.int64)
        wide = rng.integers(I32_MIN, I32_MAX + 1, size=o, dtype=np.int64)
        bias = np.where(c % 4 == 0, I32_MAX - near, np.where(c % 4 == 1, I32_MIN + near, wide)).astype(np.int32)
        zp_vec = ref.wrap_i32(bias.astype(np.int64) + zp_vec).astype(np.int32)
        return bias, _scale(m), zp_vec
    assert regime == "tensor"
    ms = 48.0 / max(float(conv.astype(np.float64).std()), 1.0)
    if mode == "TENSOR_UPWARD":
        return bias, _scale(ms)[()], np.int32(37)
    if mode == "TENSOR_POW2":
        return bias, _scale(_snap(ms))[()], zp_vec
    return bias, _scale(_snap(ms))[()], np.int32(37)


def build(name: str, regime: str, mode: str) -> Case:
    """The case of one geometry x regime x mode, with every expected record from the oracle."""
    return chain(GEOMETRY[name], regime, mode, *operands(name, regime == "small"))


def chain(g: Geometry, regime: str, mode: str, x, w, zv, conv) -> Case:
    """The case of a geometry's operands and conv record under regime x mode: the draws of _draw and
    the oracle's records after the conv."""
    name = g.name
    bias, s_in, rq_zp = _draw(g, regime, mode, conv)
    rounding = "TONEAREST" if mode.endswith("TONEAREST") else "UPWARD"
    badd = ref.bias_add(conv, bias, 1)
    rq = ref.requantize(badd, s_in, rq_zp, S_OUT, np.int32(g.zp_out), axis=1, rounding=rounding, out_dtype=g.dtype)
    exp = [conv, badd, rq]
    residual = add_params = None
    if g.residual:
        residual = _uniform(_rng(name, "residual"), rq.shape, g.dtype)
        add_params = ADD_PARAMS[g.dtype]
        exp.append(ref.qnn_add(residual, rq, *add_params) if g.block_is_rhs else ref.qnn_add(rq, residual, *add_params))
    exp.append(ref.clip(exp[-1], *g.clip))
    return Case(g, regime, mode, x, w, bias, zv, s_in, rq_zp, rounding, residual, add_params, exp,
                None if g.dense else blocked_shadow(exp[-1]))
