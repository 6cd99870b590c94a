"""The reference side of the non-square geometry tests (tests/rect_cases.py), on the CPU: every
geometry really breaks a symmetry of the two axes, the oracle's conv equals an independent float64
convolution, the oracle's records leave the kernels something to get wrong, a swap of the two axes'
attributes shows in the expected record, and the oracle's pools equal a four-loop restatement.  Seeds
are fixed, so these hold deterministically; a geometry that misses a bound gets another shape or
draw, never another bound.
"""
import numpy as np
import pytest

from oracle import qnn_ref as ref
from tests import rect_cases as rc

NAMES = [g.name for g in rc.GEOMETRIES]
KINDS = ("OH != OW", "KH != KW", "sh != sw", "dh != dw", "padding not all equal")


def _anisotropy(g):
    (kh, kw), (sh, sw), pad, (dh, dw) = rc.attrs(g)
    oh, ow = rc.out_hw(g)
    return [k for k, on in zip(KINDS, (oh != ow, kh != kw, sh != sw, dh != dw, len(set(pad)) > 1)) if on]


def test_anisotropy():
    """Every geometry breaks at least one equality of the two axes; each of the five is broken by
    at least three geometries; both lists hold an H > W and an H < W plane."""
    count = dict.fromkeys(KINDS, 0)
    for g in rc.GEOMETRIES:
        kinds = _anisotropy(g)
        print(g.name, g.x_shape, "->", rc.out_hw(g), kinds)
        assert kinds, g.name
        for k in kinds:
            count[k] += 1
    print(count)
    assert min(count.values()) >= 3, count
    for group in (rc.RECT + rc.ANISO, rc.SINGLE):
        assert any(g.x_shape[2] > g.x_shape[3] for g in group) and any(g.x_shape[2] < g.x_shape[3] for g in group)


def _torch_conv(g, x, w, zv, strides, padding, dilation):
    """The convolution in float64 through torch, zero points subtracted first and the padding made
    explicit: exact, every |sum| here is far below 2^53."""
    import torch
    import torch.nn.functional as F
    zw = (zv if zv is not None else np.full(g.o, g.zw)).astype(np.float64).reshape(-1, 1, 1, 1)
    a = torch.from_numpy(x.astype(np.float64) - g.za)
    b = torch.from_numpy(w.astype(np.float64) - zw)
    pt, pl, pb, pr = padding
    out = F.conv2d(F.pad(a, (pl, pr, pt, pb)), b, stride=strides, dilation=dilation, groups=g.groups)
    return out.numpy()


@pytest.mark.parametrize("name", NAMES)
def test_independent_conv(name):
    """The oracle's conv record equals torch.nn.functional.conv2d in float64, which shares nothing
    with the oracle's tap loop."""
    g = rc.GEOMETRY[name]
    x, w, zv, conv = rc.operands(name)
    kw = g.conv_kw
    exp = _torch_conv(g, x, w, zv, kw["strides"], kw["padding"], kw["dilation"])
    assert np.abs(exp).max() < 2 ** 31
    assert conv.shape == exp.shape == (g.x_shape[0], g.o) + rc.out_hw(g)
    np.testing.assert_array_equal(conv.astype(np.float64), exp)


@pytest.mark.parametrize("name,mode", rc.CASE_IDS, ids=["-".join(i) for i in rc.CASE_IDS])
def test_requantize_record(name, mode):
    """The bounds of test_block_value_cases.py: at least half of the requantize outputs are neither
    qmin nor qmax, and the record holds at least 200 distinct byte values (a record of fewer than
    200 elements: half its element count)."""
    rq = rc.build(name, mode).requantize_record
    lo, hi = ref.dtype_range(str(rq.dtype))
    share = float(np.mean((rq != lo) & (rq != hi)))
    distinct = len(np.unique(rq))
    print(name, mode, "unsaturated", round(share, 3), "distinct", distinct, "of", rq.size)
    assert share >= 0.5, share
    assert distinct >= (200 if rq.size >= 200 else rq.size // 2), (distinct, rq.size)


def _swaps(g):
    """(what, conv_kw, weight transposed) of every swap of the two axes' attributes: each unequal
    pair alone, all of them together, and the kernel's taps transposed where KH == KW > 1."""
    (kh, kw_), (sh, sw), (pt, pl, pb, pr), (dh, dw) = rc.attrs(g)
    base = g.conv_kw
    one = {}
    if sh != sw:
        one["strides"] = (sw, sh)
    if (pt, pb) != (pl, pr):
        one["padding"] = (pl, pt, pr, pb)
    if dh != dw:
        one["dilation"] = (dw, dh)
    out = [(k, dict(base, **{k: v}), False) for k, v in one.items()]
    if len(one) > 1:
        out.append(("+".join(one), dict(base, **one), False))
    if kh == kw_ and kh > 1:
        out.append(("kernel taps transposed", base, True))
        out += [(f"{what}, kernel taps transposed", kw, True) for what, kw, _ in out[:-1]]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_swap_shows(name):
    """Where a swap of the two axes' attributes keeps the output shape, the oracle's conv with the
    swapped attributes differs from the true one in at least a quarter of its elements: a kernel
    that swapped them cannot pass test_gpu_rect.py."""
    g = rc.GEOMETRY[name]
    x, w, zv, conv = rc.operands(name)
    h, wd = g.x_shape[2:]
    for what, kw, transposed in _swaps(g):
        wt = np.ascontiguousarray(w.transpose(0, 1, 3, 2)) if transposed else w
        kh, kw_ = wt.shape[2:]
        (sh, sw), (pt, pl, pb, pr), (dh, dw) = kw["strides"], kw["padding"], kw["dilation"]
        if h + pt + pb < dh * (kh - 1) + 1 or wd + pl + pr < dw * (kw_ - 1) + 1:
            continue
        if ((h + pt + pb - dh * (kh - 1) - 1) // sh + 1, (wd + pl + pr - dw * (kw_ - 1) - 1) // sw + 1) != conv.shape[2:]:
            print(name, what, "changes the output shape")
            continue
        swapped = ref.qnn_conv2d(x, wt, g.za, zv if zv is not None else g.zw, **kw)
        share = float(np.mean(swapped != conv))
        print(name, what, "changes", round(share, 3))
        assert share >= 0.25, (what, share)


# ---------------------------------------------------------------------------------- pools
def _wrap(v, dtype):
    """v reduced to the dtype's range (two's complement)."""
    info = np.iinfo(dtype)
    span = int(info.max) - int(info.min) + 1
    return (int(v) - int(info.min)) % span + int(info.min)


def _truncdiv(a, b):
    q = abs(a) // abs(b)
    return -q if (a < 0) != (b < 0) else q


def _pool_loops(x, kind, pool_size, strides, padding, dilation, include_pad=False):
    """nn.max_pool2d / nn.avg_pool2d restated with four loops per output element, from the kernels'
    comments (csrc/tk_elementwise.hip): taps at oh * sh - pt + r * dh, ow * sw - pl + c * dw; a
    tap outside the image is the dtype minimum for max and absent from the sum for avg; the sum
    wraps in the input dtype and is divided, truncating towards zero, by the number of window taps
    inside the image (at least 1), or inside the padded image with count_include_pad."""
    n, ch, h, w = x.shape
    (kh, kw), (sh, sw), (pt, pl, pb, pr), (dh, dw) = pool_size, strides, padding, dilation
    oh = (h + pt + pb - dh * (kh - 1) - 1) // sh + 1
    ow = (w + pl + pr - dw * (kw - 1) - 1) // sw + 1
    out = np.zeros((n, ch, oh, ow), x.dtype)
    lo = int(np.iinfo(x.dtype).min)
    xl = x.tolist()
    for b in range(n):
        for c in range(ch):
            plane = xl[b][c]
            for i in range(oh):
                for j in range(ow):
                    best, total, inside, padded = lo, 0, 0, 0
                    for r in range(kh):
                        ih = i * sh - pt + r * dh
                        for s in range(kw):
                            iw = j * sw - pl + s * dw
                            if -pt <= ih < h + pb and -pl <= iw < w + pr:
                                padded += 1
                            if 0 <= ih < h and 0 <= iw < w:
                                inside += 1
                                total += plane[ih][iw]
                                best = max(best, plane[ih][iw])
                    if kind == "max":
                        out[b, c, i, j] = best
                    else:
                        cnt = padded if include_pad else max(inside, 1)
                        out[b, c, i, j] = _wrap(_truncdiv(_wrap(total, x.dtype), cnt), x.dtype)
    return out


@pytest.mark.parametrize("dtype", list(rc.POOL_CASES))
@pytest.mark.parametrize("setting", range(len(rc.POOL_SETTINGS)))
def test_pools_against_loops(dtype, setting):
    x = rc.pool_input(dtype)
    size, strides, padding, dilation = rc.POOL_SETTINGS[setting]
    kw = dict(pool_size=size, strides=strides, padding=padding, dilation=dilation)
    np.testing.assert_array_equal(ref.max_pool2d(x, **kw), _pool_loops(x, "max", size, strides, padding, dilation))
    for include in (False, True):
        np.testing.assert_array_equal(ref.avg_pool2d(x, count_include_pad=include, **kw),
                                      _pool_loops(x, "avg", size, strides, padding, dilation, include))


@pytest.mark.parametrize("dtype", rc.GLOBAL_DTYPES)
@pytest.mark.parametrize("plane", rc.GLOBAL_PLANES, ids=lambda p: f"{p[0]}x{p[1]}")
def test_global_avg_pool_against_loops(dtype, plane):
    """nn.global_avg_pool2d: the plane's sum wrapped into the dtype, divided, truncating, by the
    element count in the same dtype (csrc/tk_elementwise.hip global_avg_kernel: 150 elements of an
    int8 plane divide by int8(150) = -106)."""
    x = rc.pool_input(dtype, (2, 5) + plane)
    exp = np.zeros((2, 5, 1, 1), x.dtype)
    for b in range(2):
        for c in range(5):
            total = sum(int(v) for row in x[b, c].tolist() for v in row)
            exp[b, c, 0, 0] = _wrap(_truncdiv(_wrap(total, x.dtype), _wrap(plane[0] * plane[1], x.dtype)), x.dtype)
    got = ref.global_avg_pool2d(x)
    print(dtype, plane, exp.ravel().tolist())
    np.testing.assert_array_equal(got, exp)


def test_shared_cases():
    """The modes of a geometry share their draws, and the cached arrays cannot be written to."""
    a, b = rc.build("dw_wide", "AXIS_UPWARD"), rc.build("dw_wide", "AXIS_TONEAREST")
    assert a.x is b.x and a.expected[0] is b.expected[0]
    assert np.array_equal(a.s_in, b.s_in) and np.array_equal(a.rq_zp, b.rq_zp) and np.array_equal(a.bias, b.bias)
    with pytest.raises(ValueError):
        a.x[0, 0, 0, 0] = 1
    assert rc.build("dw_wide", "AXIS_UPWARD") is a
