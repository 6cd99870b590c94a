"""The reference side of the fused-block value matrix (tests/block_value_cases.py), on the CPU: for
every geometry x regime the oracle's own records must leave the kernels something to get wrong --
mostly unsaturated requantize outputs, many distinct bytes, a wrapping bias add, roundings that
differ -- so that test_gpu_block_values.py cannot pass trivially.  Seeds are fixed, so these hold
deterministically; a geometry that misses a bound gets another draw, never another bound.

The distinct-value bound is 200 byte values.  One geometry the matrix has to keep, dense_5x84x10,
has a record of 50 elements, which cannot hold 200 values; there the bound is half the element
count, which no near-constant record meets either.
"""
import numpy as np
import pytest

from oracle import qnn_ref as ref
from tests import block_value_cases as bvc

NAMES = [g.name for g in bvc.GEOMETRIES]


@pytest.fixture(scope="module")
def case():
    cache = {}

    def get(name, regime, mode):
        key = (name, regime, mode)
        if key not in cache:
            cache[key] = bvc.build(*key)
        return cache[key]
    return get


def _unsaturated(rq):
    lo, hi = ref.dtype_range(str(rq.dtype))
    return float(np.mean((rq != lo) & (rq != hi)))


@pytest.mark.parametrize("name", NAMES)
def test_unsaturated_share(case, name):
    """At least half of the requantize outputs are neither qmin nor qmax, in every regime and mode."""
    shares = {(r, m): _unsaturated(case(name, r, m).requantize_record) for r, m in bvc.VARIANTS}
    print(name, {f"{r}-{m}": round(s, 3) for (r, m), s in shares.items()})
    assert min(shares.values()) >= 0.5, shares


@pytest.mark.parametrize("regime", ["calibrated", "wrap"])
@pytest.mark.parametrize("name", NAMES)
def test_distinct_values(case, name, regime):
    for mode in ("AXIS_UPWARD", "AXIS_TONEAREST"):
        rq = case(name, regime, mode).requantize_record
        distinct = len(np.unique(rq))
        print(name, regime, mode, "distinct", distinct, "of", rq.size)
        assert distinct >= (200 if rq.size >= 200 else rq.size // 2), (mode, distinct, rq.size)


@pytest.mark.parametrize("name", NAMES)
def test_wrap_share(case, name):
    """In wrap, the bias add leaves int32 in at least a tenth of the elements, and the zero-point
    subtraction brings the requantize input back to within the conv's reach."""
    c = case(name, "wrap", "AXIS_UPWARD")
    conv, badd = c.expected[0], c.expected[1]
    shape = [1, -1] + [1] * (conv.ndim - 2)
    exact = conv.astype(np.int64) + c.bias.astype(np.int64).reshape(shape)
    share = float(np.mean(exact != badd))
    print(name, "wrap share", round(share, 3))
    assert share >= 0.10, share
    back = ref.wrap_i32(badd.astype(np.int64) - c.rq_zp.astype(np.int64).reshape(shape))
    assert np.abs(back - conv).max() <= 1000


@pytest.mark.parametrize("name", NAMES)
def test_rounding_difference(case, name):
    """In small, UPWARD and TONEAREST give different records: exact ties at negative values occur."""
    up, near = (case(name, "small", m).requantize_record for m in ("AXIS_UPWARD", "AXIS_TONEAREST"))
    axis = float(np.mean(up != near))
    up, near = (case(name, "small", m).requantize_record for m in ("TENSOR_POW2", "TENSOR_TONEAREST"))
    scalar = float(np.mean(up != near))
    print(name, "rounding difference: per axis", round(axis, 4), "0.25 scalar", round(scalar, 4))
    assert axis >= 0.01, axis
    assert scalar >= 0.05, scalar


@pytest.mark.parametrize("name", NAMES)
def test_clip_bounds_and_between(case, name):
    """Both clip bounds and values strictly between them occur in the clip record of every case on
    uniform operands (the small regime's records stay inside the bounds where K is small)."""
    g = bvc.GEOMETRY[name]
    lo, hi = g.clip
    for regime, mode in bvc.VARIANTS:
        if regime == "small":
            continue
        clip = case(name, regime, mode).expected[-1]
        assert clip.min() == lo and clip.max() == hi, (regime, mode, int(clip.min()), int(clip.max()))
        assert np.any((clip > lo) & (clip < hi)), (regime, mode)


def test_shared_operands():
    """The modes of a regime share their draws, and the cached operands cannot be written to."""
    a, b = bvc.build("dw_flat", "calibrated", "AXIS_UPWARD"), bvc.build("dw_flat", "calibrated", "AXIS_TONEAREST")
    assert a.x is b.x and a.expected[0] is b.expected[0]
    assert np.array_equal(a.s_in, b.s_in) and np.array_equal(a.rq_zp, b.rq_zp) and np.array_equal(a.bias, b.bias)
    with pytest.raises(ValueError):
        a.x[0, 0, 0, 0] = 1


def test_modes():
    """requantize_plan (the library's constant folding) gives each case the mode it is named for."""
    from tachikoma_amd import _lib
    try:
        _lib.load()
    except Exception as e:  # as test_lib_load.py: only this needs the built library
        pytest.skip(f"library not built: {e}")
    from tachikoma_amd.relay.build_module import requantize_plan
    for name, regime, mode in bvc.CASE_IDS:
        g = bvc.GEOMETRY[name]
        conv = bvc.operands(name, regime == "small")[3]
        _, s_in, _ = bvc._draw(g, regime, mode, conv)
        rounding = "TONEAREST" if mode.endswith("TONEAREST") else "UPWARD"
        got = requantize_plan(s_in, bvc.S_OUT, rounding)[0]
        assert bvc.MODES[got] == mode, (name, regime, mode, bvc.MODES[got])
