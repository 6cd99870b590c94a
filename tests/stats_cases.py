"""The per-record statistics of an array in plain numpy, written from their definitions, for the
tests of tachikoma_amd's host twin (test_record_stats.py) and of the device kernel
(test_gpu_record_stats.py, test_gpu_module_stats.py): count, sum modulo 2^64, min, max,
bits[b] = elements whose magnitude has bit length b (b(0) = 0, b(x) = floor(log2|x|) + 1, 32 for
INT32_MIN), values[v - dtype_min] for the 1-byte dtypes."""
import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
KIND = {"int32": 0, "int8": 1, "uint8": 2}
DTYPE = {0: np.int32, 1: np.int8, 2: np.uint8}


def ref_fields(x):
    """(count, sum, min, max, bits, values) of one array."""
    x = np.asarray(x).reshape(-1)
    wide = x.astype(np.int64)
    length = np.searchsorted(2 ** np.arange(32, dtype=np.int64), np.abs(wide), side="right")
    bits = np.bincount(length, minlength=33).astype(np.uint64)
    values = None
    if x.dtype.itemsize == 1:
        values = np.bincount(wide - np.iinfo(x.dtype).min, minlength=256).astype(np.uint64)
    if x.size == 0:
        return 0, 0, I32_MAX, I32_MIN, bits, values
    return x.size, int(np.sum(x, dtype=np.int64)), int(wide.min()), int(wide.max()), bits, values


def ref_merged(arrays):
    """ref_fields of several arrays of one dtype taken together."""
    return ref_fields(np.concatenate([np.asarray(a).reshape(-1) for a in arrays]))


def assert_fields(s, fields, dtype, what=None):
    """A RecordStats against ref_fields' tuple, field by field."""
    count, total, lo, hi, bits, values = fields
    assert s.dtype == str(np.dtype(dtype)), what
    assert (s.count, s.sum, s.min, s.max) == (count, total, lo, hi), (what, s.count, s.sum, s.min, s.max, fields[:4])
    assert s.bits.dtype == np.uint64 and s.bits.shape == (33,) and np.array_equal(s.bits, bits), (what, s.bits, bits)
    assert int(s.bits.sum()) == count, what
    if values is None:
        assert s.values is None, what
    else:
        assert s.values.dtype == np.uint64 and s.values.shape == (256,), what
        assert np.array_equal(s.values, values), (what, np.flatnonzero(s.values != values)[:8])
        assert int(s.values.sum()) == count, what


def assert_is(s, x, what=None):
    assert_fields(s, ref_fields(x), np.asarray(x).dtype, what)


def contents(kind, n, rng):
    """The contents the kernel is tried on, {label: array of n elements}: the full range with the
    extremes at both ends, small values around zero, all zeros, all the dtype's minimum, ninety
    percent zeros."""
    dt = np.dtype(DTYPE[kind])
    info = np.iinfo(dt)
    full = rng.integers(info.min, info.max, n, dtype=np.int64, endpoint=True).astype(dt)
    planted = full.copy()
    if n:
        planted[0], planted[-1] = info.min, info.max
    sparse = full.copy()
    sparse[rng.random(n) < 0.9] = 0
    return {"extremes": planted,
            "small": rng.integers(max(info.min, -3), 3, n, endpoint=True).astype(dt),
            "zeros": np.zeros(n, dt),
            "all_min": np.full(n, info.min, dt),
            "sparse": sparse}
