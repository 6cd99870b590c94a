"""Host side of the device calibration (relay.quantize.passes): kl_threshold is the tail of
find_scale_by_kl, radix_select with a numpy counter is np.partition, histogram_edges are
np.histogram's edges.  No GPU."""
import numpy as np
import pytest

from tachikoma_amd.relay.quantize import passes
from tests.float_stats_cases import numpy_digit_counter, select_cases


def _kl_arrays():
    rng = np.random.default_rng(8)  # the arrays of tests/test_quantize.py's KL tests
    out = [d.astype(np.float32) for d in (rng.standard_normal(5000), np.abs(rng.standard_normal(5000)),
                                          rng.laplace(size=5000) * 3)]
    out.append((np.random.default_rng(9).standard_normal(20000) * 2.5).astype(np.float32))
    out.append(np.random.default_rng(0).standard_normal(10000).astype(np.float32))
    return out


@pytest.mark.parametrize("qdtype", ["int8", "uint8"])
@pytest.mark.parametrize("bins,qbins", [(8001, 255), (201, 21)])
def test_kl_threshold_is_the_tail_of_find_scale_by_kl(qdtype, bins, qbins):
    seen_nonneg = False
    for arr in _kl_arrays():
        mn, mx = np.min(arr), np.max(arr)
        thres = max(abs(mn), abs(mx))
        hist, edges = np.histogram(arr, bins=bins, range=(-thres, thres))
        want = passes.find_scale_by_kl(arr, qdtype, bins, qbins)
        assert passes.kl_threshold(hist, edges, mn, qdtype, bins, qbins) == want
        # the device path's form of the same counts and edges: uint64 counts, histogram_edges
        e2 = passes.histogram_edges(mn, mx, bins)
        assert e2.dtype == np.float32 and np.array_equal(e2.view(np.uint32), edges.view(np.uint32))
        assert passes.kl_threshold(hist.astype(np.uint64), e2, mn, qdtype, bins, qbins) == want
        seen_nonneg |= bool(mn >= 0)
    assert seen_nonneg  # the uint8 case with min >= 0 doubles the quantized bins


def test_kl_threshold_uint8_nonnegative_differs_from_int8():
    arr = np.abs(np.random.default_rng(8).standard_normal(5000)).astype(np.float32)
    assert np.min(arr) >= 0
    hist, edges = np.histogram(arr, bins=8001, range=(-np.max(arr), np.max(arr)))
    u8 = passes.kl_threshold(hist, edges, np.min(arr), "uint8")
    assert u8 == passes.find_scale_by_kl(arr, "uint8")
    # 511 quantized bins, not 255: the call really took the uint8 branch
    assert u8 == passes.kl_threshold(hist, edges, np.float32(-1), "int8", 8001, 511)


@pytest.mark.parametrize("name", sorted(select_cases(4099)))
def test_radix_select_equals_partition(name):
    x = select_cases(4099)[name]
    n = x.size
    mag = np.abs(x)
    for k in sorted({0, n - 1, int(n * 0.99999)}):
        want = np.partition(mag, k)[k]
        got = passes.radix_select(numpy_digit_counter([x]), [k])
        assert got == [int(want.view(np.uint32))], (name, k)
    # several records at once, and the rank as a function of the count
    other = select_cases(513)[name]
    got = passes.radix_select(numpy_digit_counter([x, other]), lambda total: int(total * 0.99999))
    for g, y in zip(got, (x, other)):
        k = int(y.size * 0.99999)
        assert g == int(np.partition(np.abs(y), k)[k].view(np.uint32))


def test_radix_select_refuses_a_rank_outside_the_record():
    x = np.ones(10, np.float32)
    with pytest.raises(ValueError):
        passes.radix_select(numpy_digit_counter([x]), [10])
    with pytest.raises(ValueError):
        passes.radix_select(numpy_digit_counter([x[:0]]), [0])


def test_radix_select_sees_nonfinite_values_in_the_top_digits():
    x = np.array([1.0, np.inf, -np.inf, np.nan, 2.0], np.float32)
    table = numpy_digit_counter([x])(0, None)[0]
    assert int(table[0x7F8:].sum()) == 3 and int(table.sum()) == 5


@pytest.mark.parametrize("bins", [2, 11, 255, 8001, 8192])
def test_histogram_edges_are_numpys(bins):
    rng = np.random.default_rng(3)
    records = [rng.standard_normal(1000).astype(np.float32) * s for s in (1e-3, 1.0, 1e4)]
    records += [np.maximum(rng.standard_normal(1000), 0).astype(np.float32), np.zeros(100, np.float32),
                np.full(7, -2.5, np.float32), np.array([1e-42, -3e-41], np.float32)]
    for x in records:
        mn, mx = np.min(x), np.max(x)
        thres = max(abs(mn), abs(mx))
        want = np.histogram(x, bins=bins, range=(-thres, thres))[1]
        got = passes.histogram_edges(mn, mx, bins)
        assert got.dtype == want.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    z = passes.histogram_edges(np.float32(0), np.float32(-0.0), bins)
    assert z[0] == -0.5 and z[-1] == 0.5  # numpy's widening of an all-zero record
