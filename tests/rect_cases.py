"""Shared cases of the non-square geometry tests (CPU reference checks in test_rect_cases.py, the
kernels in test_gpu_rect.py).  Every other GPU test of a fused block has H == W, KH == KW,
sh == sw, dh == dw and one padding on all four sides, so a kernel that swapped one of these pairs
would pass them; here each geometry breaks at least one of the equalities.

A geometry is a block_value_cases.Geometry whose k / stride / dilation may be pairs and whose pad
may be (top, left, bottom, right).  Its inputs are drawn as the `calibrated` regime of
block_value_cases draws them (uniform 8-bit operands, bias in +-2^14, M[c] = 48 / sigma_c * U[0.5, 2]
with every 8th channel snapped to a power of two, a vector of requantize input zero points,
s_out = 0.05, clip (lo + 40, hi - 30)) and every expected record comes from oracle.qnn_ref through
block_value_cases.chain.  All geometries run under AXIS_UPWARD, those of TONEAREST under
AXIS_TONEAREST too (algos 3 and 4 are listed only under UPWARD, so TONEAREST takes the same shape
through the general epilogue).

Three lists:
  RECT    MFMA blocks with a square 3x3 pad 1 or 1x1 pad 0 conv on a rectangular plane; each keeps the
          pixel count of the square shape that reaches its kernel family in block_value_cases.
  ANISO   MFMA blocks with an unequal kernel, stride, dilation or padding: the image-tile plans decline
          them, the im2col families run.
  SINGLE  depthwise, grouped and tiny-Cin blocks: one kernel, tk_conv2d_block_algos lists nothing.
          Which kernel, and which of its branches, is in each case's comment (read from
          dw_block_try in csrc/tk_dw.hip and conv_direct_run in csrc/tk_conv_direct.hip; the kernel names are those
          of profiles/rect_dw_kernel_trace.txt).

What the reference alone gives (test_rect_cases.py asserts the bounds in brackets per geometry; the
minima over all geometries, with the geometry that sets them):
  unsaturated share of the requantize record [>= 0.5]: 0.879 (dw_wide); next 0.905 (dw_flat_rect)
  distinct byte values [>= 200; a record of fewer than 200 elements: half its element count]:
      238 (direct_5x3, 1440 elements), 250 (dw_direct_s21, 2240), 251 (dw_direct_3x5_dil, u8_zw_rect);
      no record here has fewer than 200 elements
  share of the conv record that a swap of the two axes' attributes changes [>= 0.25]: above 0.999 in
      each of the 28 swaps that keep the output shape (strides, padding, dilation, each alone and
      together, and the kernel's taps transposed where KH == KW > 1); 30 more change the shape

POOL_CASES / POOL_SETTINGS / GLOBAL_PLANES are the pool inputs of both test files.
"""
import functools

import numpy as np

from oracle import qnn_ref as ref
from tests import block_value_cases as bvc
from tests.block_value_cases import Geometry

SEED = 1  # of the operand draws (bias, scales and zero points come from block_value_cases._draw)
MODES = ("AXIS_UPWARD", "AXIS_TONEAREST")


def _dw(name, meant, x_shape, **kw):
    return Geometry(name, meant, x_shape, x_shape[1], groups=x_shape[1], **kw)


RECT = [
    Geometry("rect_img3x3_wide", "3x3 image tiles, several images per workgroup, last partial, H < W",
             (3, 64, 7, 28), 64, k=3, pad=1),
    Geometry("rect_img3x3_tall", "as rect_img3x3_wide, H > W", (3, 64, 28, 7), 64, k=3, pad=1),
    Geometry("rect_img3x3_s2", "strided halo patch: odd H, even W -> 7x14", (2, 64, 13, 28), 64, k=3, stride=2, pad=1,
             dtype="uint8"),
    Geometry("rect_img3x3_oddrow", "hw % 4 == 0 with odd OW: every 4-vector of a record crosses a row",
             (3, 64, 4, 49), 64, k=3, pad=1),
    Geometry("rect_stage128_1x1", "128-channel stages; persistent algos 3 and 4 under UPWARD", (2, 128, 8, 18), 64),
    Geometry("rect_stage128_1x1_res", "as rect_stage128_1x1, transposed, with a residual join, the block on the rhs",
             (2, 128, 18, 8), 64, residual=True, block_is_rhs=True),
    Geometry("rect_1x1_s2", "strided patch loader of a 1x1 -> 6x14", (2, 128, 12, 28), 128, stride=2),
    Geometry("rect_split_img_160", "split-K image plans, odd hw (45)", (4, 160, 5, 9), 64, k=3, pad=1),
    Geometry("rect_split_im2col_256", "split-K im2col", (2, 256, 9, 5), 64, k=3, pad=1),
    Geometry("rect_rows128_512", "128-row tiles", (2, 512, 5, 20), 128),
    Geometry("rect_cols256_1024", "256-column tiles (a grid of >= 256 tiles)", (16, 64, 7, 28), 1024),
    Geometry("rect_chunk32_144_u8_res", "weight-stationary 1x1, partial 32-row chunk, uint8, residual join",
             (3, 24, 14, 56), 144, dtype="uint8", residual=True),
    Geometry("rect_small_planes", "planes of <= 64 pixels, 12 images per tile, last tile partial", (40, 32, 2, 5), 64,
             k=3, pad=1),
]

ANISO = [
    Geometry("k1x7", "taps = 7 along W, 128-byte stages, hw = 144: algos 3 and 4 too", (2, 128, 6, 24), 64, k=(1, 7),
             pad=(0, 3, 0, 3)),
    Geometry("k7x1", "taps = 7 along H", (2, 64, 24, 6), 64, k=(7, 1), pad=(3, 0, 3, 0)),
    Geometry("k3x5_s21", "cin_pad 32: the general im2col walk, ragged O", (2, 32, 17, 12), 48, k=(3, 5), stride=(2, 1),
             pad=(1, 2, 0, 2)),
    Geometry("dil21_s12", "unequal dilation and stride", (2, 32, 12, 20), 48, k=3, stride=(1, 2), dilation=(2, 1),
             pad=(2, 1, 2, 1)),
    Geometry("dil13_same", "dilation along W only, on 64-channel stages", (2, 64, 9, 16), 64, k=3, dilation=(1, 3),
             pad=(1, 3, 1, 3)),
    Geometry("same_s2", "TF SAME padding at stride 2: the image plans decline, im2col runs", (2, 64, 14, 30), 64, k=3,
             stride=2, pad=(0, 0, 1, 1)),
    Geometry("s12_1x1", "1x1 with stride along W only: 10x14 outputs, hw % 4 == 0", (2, 64, 10, 28), 64,
             stride=(1, 2)),
    Geometry("u8_zw_rect", "per-pixel patch sums (scratch) on an odd plane: uint8 data and weights, zw 127",
             (1, 32, 6, 11), 32, k=3, pad=(1, 0, 1, 2), dtype="uint8", w_dtype="uint8", zw=127),
]

SINGLE = [
    # dw_tile_kernel<kDwRow1>: OW = 56 (% 4 == 0), pl = 1; one whole plane of 784 pixels per tile,
    # one channel group (16 * 2 * 784 > 4096); W % 16 == 8: 8-byte row loads, Wp = 96, 16 staged rows
    _dw("dw_wide", "tile kernel, whole planes, kDwRow1 (OW % 4 == 0)", (2, 32, 14, 56), k=3, pad=1),
    # dw_tile_kernel<kDwGen>: OW = 14; 1148 pixels > 1024, so bands of 36, 36 and 10 rows (82 has no
    # divisor in [18, 36]; 36 * 14 and 10 * 14 are multiples of 4); bands are never staged flat, so
    # the rows come through the 2-byte loads (W % 4 == 2), Wp = 48, 38 staged rows
    _dw("dw_tall", "tile kernel, kDwGen, row bands staged with vw = 2", (2, 16, 82, 14), k=3, pad=1),
    # dw_tile_kernel<kDwRow1>: OW = 72; 2952 pixels: bands of 7 rows (41 is prime), the sixth band
    # has 6; 8-byte row loads, Wp = 96, 9 staged rows
    _dw("dw_bands_wide", "tile kernel, row bands, last band partial", (2, 16, 41, 72), k=3, pad=1),
    # dw_tile_kernel<kDwRow2>: 45x20 outputs; a whole plane would stage 91 rows of 80 bytes for 16
    # channels (over 64 KB of LDS), so 5 bands of 9 rows, 19 staged rows each; 8-byte row loads
    _dw("dw_bands_tall_s2", "tile kernel, kDwRow2, bands", (2, 16, 90, 40), k=3, stride=2, pad=1),
    # dw_tile_kernel<kDwGen> (pl = 0): 15x7 outputs, two channel groups per tile, 31 staged rows from
    # input row 0 (row 30 keeps the zero-point fill: the bottom padding), Wp = 48: the last tap
    # column, 14, is the fill right of the 14 image bytes; staged flat (W % 8 != 0)
    _dw("dw_same_s2_u8", "tile kernel with top/left padding 0, bottom/right 1 (TF SAME at stride 2), uint8, "
        "per-channel kernel zero points", (2, 32, 30, 14), k=3, stride=2, pad=(0, 0, 1, 1), dtype="uint8", zw_vec=True),
    # dw_tile_kernel<kDwGen> (pl = 0): 12x20 outputs, 14 staged rows from input row -2, Wp = 64
    # (tap columns reach 21, the fill right of the 20 image bytes); staged flat (W % 8 == 4)
    _dw("dw_pad_2002", "unequal padding within the tile kernel's bounds", (2, 16, 12, 20), k=3, pad=(2, 0, 0, 2)),
    # dw_tile_kernel<kDwGen>: 45 pixels, four channel groups per tile (64 * 45 elements), staged flat,
    # the shadow written pixel by pixel (45 % 4 != 0)
    _dw("dw_flat_rect", "tile kernel, flat staging, four channel groups per tile", (2, 64, 5, 9), k=3, pad=1),
    # dw3x3_kernel<4> (sh != sw: dw_block_try declines): 28x32 outputs, 896 pixels >= 784 at sh = 1,
    # one whole plane per workgroup, 30 staged rows of 72 bytes; the last tap column is
    # 31 * 2 + 2 + 4 - 1 = 67 < 72
    _dw("dw_band_s12", "band kernel with sh = 1, sw = 2", (1, 16, 28, 64), k=3, stride=(1, 2), pad=1),
    # dw3x3_kernel<4>: 56x60 outputs, 3360 pixels >= 3136; bands of 256 / 60 = 4 rows, 14 of them,
    # 9 staged rows of 68 bytes; the last tap column is 59 + 2 + 4 - 1 = 64 < 68
    _dw("dw_band_s21", "band kernel with sh = 2, sw = 1, 14 bands of 4 rows", (1, 16, 112, 60), k=3, stride=(2, 1),
        pad=1),
    # direct_conv_kernel: 5x14 outputs, too few for the band kernel
    _dw("dw_direct_s21", "direct kernel, depthwise, sh = 2, sw = 1", (2, 16, 9, 14), k=3, stride=(2, 1), pad=1),
    # direct_conv_kernel (KW = 5 and dilation: both depthwise kernels decline)
    _dw("dw_direct_3x5_dil", "direct kernel, unequal kernel and dilation", (1, 16, 10, 13), k=(3, 5), dilation=(1, 2),
        pad=(1, 4, 1, 4)),
    # direct_conv_kernel (groups = 4)
    Geometry("grouped_rect", "direct kernel, grouped, uint8", (1, 32, 9, 13), 64, k=3, stride=(2, 1), pad=1, groups=4,
             dtype="uint8"),
    # direct_conv_kernel (Cin = 1)
    Geometry("direct_5x3", "direct kernel, tiny Cin, 5x3 taps", (1, 1, 12, 20), 6, k=(5, 3), pad=(2, 1, 2, 1)),
]

GEOMETRIES = RECT + ANISO + SINGLE
GEOMETRY = {g.name: g for g in GEOMETRIES}
assert len(GEOMETRY) == len(GEOMETRIES)
TONEAREST = ("rect_img3x3_wide", "rect_stage128_1x1", "k1x7", "dw_wide")
CASE_IDS = [(g.name, m) for g in GEOMETRIES for m in MODES if m == "AXIS_UPWARD" or g.name in TONEAREST]
# the un-fused tk_qnn_conv2d runs on these
PLAIN = ("k1x7", "k7x1", "k3x5_s21", "dil21_s12", "same_s2", "u8_zw_rect", "rect_split_im2col_256", "dw_same_s2_u8",
         "grouped_rect", "direct_5x3")


def attrs(g: Geometry):
    """((KH, KW), (sh, sw), (pt, pl, pb, pr), (dh, dw)) of a geometry."""
    kw = g.conv_kw
    return g.w_shape[2:], kw["strides"], kw["padding"], kw["dilation"]


def out_hw(g: Geometry):
    (kh, kw), (sh, sw), (pt, pl, pb, pr), (dh, dw) = attrs(g)
    h, w = g.x_shape[2:]
    return (h + pt + pb - dh * (kh - 1) - 1) // sh + 1, (w + pl + pr - dw * (kw - 1) - 1) // sw + 1


@functools.lru_cache(maxsize=None)
def operands(name: str):
    """(x, w, zw_vec, conv record) of a geometry, as block_value_cases.operands draws the uniform
    ones; computed once and read-only."""
    g = GEOMETRY[name]
    rng = bvc._rng("rect", SEED, name)
    x = bvc._uniform(rng, g.x_shape, g.dtype)
    w = bvc._uniform(rng, g.w_shape, g.w_dtype)
    zv = rng.integers(-6, 7, size=g.o).astype(np.int32) if g.zw_vec else None
    conv = ref.qnn_conv2d(x, w, g.za, zv if zv is not None else g.zw, **g.conv_kw)
    for a in (x, w, zv, conv):
        if a is not None:
            a.setflags(write=False)
    return x, w, zv, conv


@functools.lru_cache(maxsize=None)
def build(name: str, mode: str) -> bvc.Case:
    """The case of one geometry x mode, every expected record from the oracle.  Shared between the
    tests that need it: its arrays must not be written to."""
    return bvc.chain(GEOMETRY[name], "calibrated", mode, *operands(name))


# ---------------------------------------------------------------------------------- pools
# (pool_size, strides, padding (top, left, bottom, right), dilation)
POOL_SETTINGS = [
    ((3, 2), (2, 1), (1, 0, 0, 1), (1, 1)),
    ((2, 3), (1, 2), (0, 1, 1, 0), (1, 1)),
    ((3, 3), (1, 1), (0, 0, 0, 0), (2, 1)),
    ((3, 3), (1, 2), (0, 0, 0, 0), (1, 2)),
]
POOL_CASES = {"int8": (2, 5, 13, 22), "uint8": (2, 5, 13, 22), "int32": (2, 5, 11, 17)}
POOL_SHADOW_CASES = {"int8": (2, 40, 13, 22), "uint8": (1, 24, 9, 14)}   # with POOL_SETTINGS[:2]
GLOBAL_PLANES = [(5, 13), (4, 16), (7, 9), (3, 50)]                        # 65, 64, 63 and 150 elements
GLOBAL_DTYPES = ("int32", "int8")


@functools.lru_cache(maxsize=None)
def pool_input(dtype: str, shape=None):
    """Uniform over the dtype (int32: over all 32 bits, so that window sums wrap); read-only."""
    x = bvc._uniform(bvc._rng("rect", SEED, "pool", dtype, shape), shape or POOL_CASES[dtype], dtype)
    x.setflags(write=False)
    return x
