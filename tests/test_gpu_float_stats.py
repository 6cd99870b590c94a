"""Float statistics on the MI355X (csrc/tk_fstats.hip): the range, edge-histogram and digit passes
through their C ABI against numpy (np.min / np.max, np.histogram, np.partition), the accumulator
of a module, and relay.quantize's device calibration against its host path.  Every result is
determined by integers -- counts, float32 bit patterns -- so every check is equality.  Element
counts sit on the edges of the kernel's geometry (a lane's 16 bytes, 256 lanes, the span S a
workgroup walks before it flushes); buffers are 16-byte aligned or 4 bytes past that."""
import ctypes

import numpy as np
import pytest

from tachikoma_amd import _lib, relay, zoo
from tachikoma_amd.contrib import graph_executor
from tachikoma_amd.contrib.trace_device import RANGE_DTYPE
from tachikoma_amd.relay.quantize import passes, qconfig, quantize
from tests import float_stats_cases as fc

pytestmark = pytest.mark.gpu

INVALID = -1  # TK_ERR_INVALID_ARG
BINS = [2, 11, 255, 8001, 8192]


@pytest.fixture(scope="module")
def lib(device):
    return _lib.load()


def _sizes(lib):
    s = lib.tk_fstats_span()
    assert s > 4097 and s % 1024 == 0
    return [0, 1, 3, 4, 5, 4095, 4096, 4097, s - 1, s, s + 1, 2 * s + 17]


class Arena:
    """float32 records in one device buffer, each 0 or 4 bytes past a 64-byte boundary."""

    def __init__(self):
        self.parts, self.at, self.size = [], [], 0

    def add(self, x, offset=0):
        raw = np.ascontiguousarray(x, np.float32).reshape(-1).view(np.uint8)
        start = self.size + offset
        self.parts.append((start, raw))
        self.at.append(start)
        self.size = (start + raw.size + 63) // 64 * 64 + 64

    def upload(self, device):
        import torch
        host = np.zeros(max(64, self.size), np.uint8)
        for start, raw in self.parts:
            host[start:start + raw.size] = raw
        self.dev = torch.from_numpy(host).to(device)
        assert self.dev.data_ptr() % 64 == 0
        return [self.dev.data_ptr() + a for a in self.at]


def _upload(device, arrays, offsets=None):
    arena = Arena()
    for i, x in enumerate(arrays):
        arena.add(x, offsets[i] if offsets else 0)
    return arena, arena.upload(device)


def _args(ptrs, arrays):
    n = len(ptrs)
    return (ctypes.c_void_p * n)(*ptrs), (ctypes.c_int64 * n)(*[int(np.size(x)) for x in arrays]), n


def _stream():
    return ctypes.c_void_p(_lib.stream_handle())


def _ok(lib, rc):
    assert rc == 0, lib.tk_last_error().decode()


def _ranges(lib, ptrs, arrays):
    src, cnt, n = _args(ptrs, arrays)
    out = np.zeros(n, RANGE_DTYPE)
    _ok(lib, lib.tk_float_range_batch(src, cnt, n, ctypes.c_void_p(out.ctypes.data), _stream()))
    return out


def _assert_range(row, x, label):
    x = np.asarray(x, np.float32).reshape(-1)
    fin = x[np.isfinite(x)]
    assert int(row["count"]) == x.size and int(row["nonfinite"]) == x.size - fin.size, label
    want = (fin.min(), fin.max()) if fin.size else (np.float32(np.inf), np.float32(-np.inf))
    assert (row["min"], row["max"]) == want, (label, row, want)


def _edges_of(x, bins, shrink=1.0):
    fin = np.asarray(x, np.float32).reshape(-1)
    fin = fin[np.isfinite(fin)]
    if not fin.size:
        return passes.histogram_edges(-1, 1, bins)
    return passes.histogram_edges(fin.min() * np.float32(shrink), fin.max() * np.float32(shrink), bins)


def _numpy_hist(x, edges):
    return np.histogram(np.asarray(x, np.float32).reshape(-1), bins=edges.size - 1, range=(edges[0], edges[-1]))[0]


def _hist(lib, ptrs, arrays, edges, bins):
    src, cnt, n = _args(ptrs, arrays)
    e = np.ascontiguousarray(np.stack(edges), np.float32)
    assert e.shape == (n, bins + 1)
    out = np.zeros((n, bins), np.uint64)
    _ok(lib, lib.tk_float_histogram_batch(src, cnt, n, ctypes.c_void_p(e.ctypes.data), bins,
                                          ctypes.c_void_p(out.ctypes.data), _stream()))
    return out


def _normal(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


def test_struct_size(lib):
    assert ctypes.sizeof(_lib.tk_float_range) == lib.tk_float_range_size() == RANGE_DTYPE.itemsize == 24


# ---------------------------------------------------------------- range

def test_range_over_sizes_and_alignments(lib, device):
    """Every size at both alignments in one launch; the record of no elements keeps the identity."""
    arrays, offsets = [], []
    for i, n in enumerate(_sizes(lib)):
        for off in (0, 4):
            arrays.append(_normal(n, 100 + i, 3.0) - np.float32(0.25))
            offsets.append(off)
    arena, ptrs = _upload(device, arrays, offsets)
    rows = _ranges(lib, ptrs, arrays)
    for row, x, off in zip(rows, arrays, offsets):
        _assert_range(row, x, (x.size, off))
    assert rows[0]["count"] == 0 and rows[0]["min"] == np.inf and rows[0]["max"] == -np.inf


def test_range_special_values(lib, device):
    s = lib.tk_fstats_span()
    big = _normal(s + 9, 1)
    big[[0, 5, s - 1, s, s + 8]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    arrays = [
        np.array([fc.FLT_MAX, -fc.FLT_MAX, 1.0], np.float32),
        np.array([fc.DENORMAL, 3 * fc.DENORMAL, 1e-40], np.float32),      # the minimum is a denormal
        np.array([-fc.DENORMAL, -1e-40, -1e-39, -5e-39], np.float32),     # the maximum is a negative denormal
        np.array([-0.0, -0.0, -0.0], np.float32),
        np.array([-0.0, -1.0], np.float32),
        np.array([np.nan, np.inf, -np.inf], np.float32),                  # no finite value: the identity
        np.array([np.nan, 2.5, np.inf, -7.0, -np.inf, np.nan, 1.0], np.float32),
        big, -np.abs(_normal(4099, 2)) - 1, np.abs(_normal(4099, 3)) + 1,
    ]
    arena, ptrs = _upload(device, arrays)
    rows = _ranges(lib, ptrs, arrays)
    for i, (row, x) in enumerate(zip(rows, arrays)):
        _assert_range(row, x, i)
    assert np.signbit(rows[3]["min"]) and np.signbit(rows[3]["max"]) and rows[3]["max"] == 0
    assert np.signbit(rows[4]["max"]) and rows[4]["max"] == 0  # -0.0 is a value of its own, not +0.0
    assert rows[5]["nonfinite"] == 3 and rows[5]["min"] == np.inf and rows[5]["max"] == -np.inf


def test_range_calls_accumulate(lib, device):
    """Two plans into one array: equal to one call over the concatenation, whatever the order of
    the signs (min and max merge through integer atomics chosen by the sign)."""
    import torch
    s = lib.tk_fstats_span()
    first = [np.abs(_normal(s + 3, 4)) + 2, -np.abs(_normal(77, 5)) - 2, _normal(4097, 6), np.zeros(0, np.float32)]
    second = [-np.abs(_normal(901, 7)) - 1, np.abs(_normal(s + 3, 8)) + 1, _normal(5, 9) * 50, _normal(3, 10)]
    second[2][1] = np.nan
    a1, p1 = _upload(device, first)
    a2, p2 = _upload(device, second)
    n = len(first)
    dev = torch.empty(3 * n, dtype=torch.int64, device=device)
    plans = []
    _ok(lib, lib.tk_float_range_reset(ctypes.c_void_p(dev.data_ptr()), n, _stream()))
    for ptrs, arrays in ((p1, first), (p2, second)):
        src, cnt, _ = _args(ptrs, arrays)
        plan = ctypes.c_void_p()
        _ok(lib, lib.tk_fstats_plan_create(src, cnt, n, ctypes.byref(plan)))
        plans.append(plan)
        _ok(lib, lib.tk_fstats_plan_range(plan, ctypes.c_void_p(dev.data_ptr()), _stream()))
    rows = dev.cpu().numpy().view(RANGE_DTYPE)
    for plan in plans:
        lib.tk_fstats_plan_destroy(plan)
    for i in range(n):
        _assert_range(rows[i], np.concatenate([first[i], second[i]]), i)


# ---------------------------------------------------------------- histogram

def _relu(n, seed):
    return np.maximum(_normal(n, seed), 0).astype(np.float32)


def _on_every_edge(x, bins):
    """x with every edge of its histogram and the edge's two float32 neighbours appended."""
    e = _edges_of(x, bins)
    return np.concatenate([x, e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))])


@pytest.mark.parametrize("bins", BINS)
def test_histogram_equals_numpy(lib, device, bins):
    """One launch over records with their own edges: data at three scales, ReLU data, all zeros, a
    constant, values on and next to every edge, and every size at both alignments."""
    sizes = _sizes(lib)
    arrays = [_normal(5000, 11, 1e-3), _normal(5000, 12), _normal(5000, 13, 1e4), _relu(sizes[-1], 14),
              np.zeros(4099, np.float32), np.full(4099, 0.75, np.float32), _normal(5000, 17, 1e-38)]  # the last: edges a few denormals apart
    edges = [_edges_of(x, bins) for x in arrays]
    offsets = [0] * len(arrays)
    for x in (_normal(3000, 15, 0.02), _relu(3000, 16), np.zeros(10, np.float32)):
        arrays.append(_on_every_edge(x, bins))
        edges.append(_edges_of(x, bins))
        offsets.append(4 * (len(arrays) % 2))
    for i, n in enumerate(sizes):
        for off in (0, 4):
            x = _relu(n, 20 + i) - np.float32(0.1) if i % 2 else _normal(n, 20 + i)
            arrays.append(x)
            edges.append(_edges_of(x, bins))
            offsets.append(off)
    arena, ptrs = _upload(device, arrays, offsets)
    got = _hist(lib, ptrs, arrays, edges, bins)
    for i, (x, e) in enumerate(zip(arrays, edges)):
        want = _numpy_hist(x, e)
        assert np.array_equal(got[i], want.astype(np.uint64)), (i, x.size, offsets[i])
        if x.size and i < 7:
            assert int(got[i].sum()) == x.size


@pytest.mark.parametrize("bins", [11, 8001])
def test_histogram_counts_nothing_outside_the_edges(lib, device, bins):
    """Edges of half the data's range: values beyond them, NaN and +-inf are counted nowhere."""
    s = lib.tk_fstats_span()
    x = _normal(s + 5, 30)
    x[[1, 100, s + 1]] = [np.nan, np.inf, -np.inf]
    y = _relu(4097, 31)
    arrays = [x, y]
    edges = [_edges_of(x, bins, 0.5), _edges_of(y, bins, 0.25)]
    arena, ptrs = _upload(device, arrays, [0, 4])
    got = _hist(lib, ptrs, arrays, edges, bins)
    for i in range(2):
        want = _numpy_hist(arrays[i], edges[i])
        assert np.array_equal(got[i], want.astype(np.uint64))
        assert 0 < int(got[i].sum()) == int(want.sum()) < arrays[i].size


def test_histogram_calls_accumulate(lib, device):
    import torch
    bins = 8001
    s = lib.tk_fstats_span()
    first, second = [_relu(s + 7, 40), _normal(300, 41)], [_relu(999, 42) * 2, _normal(s + 7, 43) * 3]
    both = [np.concatenate(p) for p in zip(first, second)]
    edges = np.stack([_edges_of(x, bins) for x in both])
    a1, p1 = _upload(device, first)
    a2, p2 = _upload(device, second, [4, 0])
    e_dev = torch.from_numpy(edges).to(device)
    h_dev = torch.zeros(2 * bins, dtype=torch.int64, device=device)
    plans = []
    for ptrs, arrays in ((p1, first), (p2, second)):
        src, cnt, n = _args(ptrs, arrays)
        plan = ctypes.c_void_p()
        _ok(lib, lib.tk_fstats_plan_create(src, cnt, n, ctypes.byref(plan)))
        plans.append(plan)
        _ok(lib, lib.tk_fstats_plan_histogram(plan, ctypes.c_void_p(e_dev.data_ptr()), bins,
                                              ctypes.c_void_p(h_dev.data_ptr()), _stream()))
    got = h_dev.cpu().numpy().view(np.uint64).reshape(2, bins)
    for plan in plans:
        lib.tk_fstats_plan_destroy(plan)
    for i in range(2):
        assert np.array_equal(got[i], _numpy_hist(both[i], edges[i]).astype(np.uint64))


# ---------------------------------------------------------------- digits and the selection driver

def test_radix_select_on_device_equals_partition(lib, device):
    """The CPU test's records at a size that crosses a span, all in one launch per level."""
    n = lib.tk_fstats_span() + 1037
    cases = fc.select_cases(n)
    labels = sorted(cases)
    arrays = [cases[k] for k in labels]
    arena, ptrs = _upload(device, arrays, [4 * (i % 2) for i in range(len(arrays))])
    src, cnt, m = _args(ptrs, arrays)

    def count(level, prefixes):
        pre = np.array([0] * m if prefixes is None else prefixes, np.uint32)
        out = np.zeros((m, 2048), np.uint64)
        _ok(lib, lib.tk_float_digits_batch(src, cnt, m, level, ctypes.c_void_p(pre.ctypes.data),
                                           ctypes.c_void_p(out.ctypes.data), _stream()))
        want = [fc.numpy_digits(x, level, int(p)) for x, p in zip(arrays, pre)]
        assert np.array_equal(out, np.stack(want)), level
        return [row[:2048 if level == 0 else 1024] for row in out]

    for k in (0, n - 1, int(n * 0.99999)):
        got = passes.radix_select(count, [k] * m)
        for label, x, g in zip(labels, arrays, got):
            assert g == int(np.partition(np.abs(x), k)[k].view(np.uint32)), (label, k)


def test_digits_of_nonfinite_values(lib, device):
    x = np.array([1.0, np.inf, -np.inf, np.nan, -0.0, 0.0, 2.0], np.float32)
    arena, ptrs = _upload(device, [x])
    src, cnt, m = _args(ptrs, [x])
    pre = np.zeros(1, np.uint32)
    out = np.zeros((1, 2048), np.uint64)
    _ok(lib, lib.tk_float_digits_batch(src, cnt, m, 0, ctypes.c_void_p(pre.ctypes.data),
                                       ctypes.c_void_p(out.ctypes.data), _stream()))
    assert np.array_equal(out[0], fc.numpy_digits(x, 0, 0))
    assert int(out[0, 0x7F8:].sum()) == 3 and int(out[0, 0]) == 2


# ---------------------------------------------------------------- refusals

def test_refusals(lib, device):
    x = _normal(100, 50)
    arena, ptrs = _upload(device, [x])
    src, cnt, n = _args(ptrs, [x])
    plan = ctypes.c_void_p()
    out = np.zeros(8192 * 2, np.uint64)
    o = ctypes.c_void_p(out.ctypes.data)
    some_edges = np.zeros(8194, np.float32)
    e = ctypes.c_void_p(some_edges.ctypes.data)
    assert lib.tk_fstats_plan_create(None, cnt, n, ctypes.byref(plan)) == INVALID
    assert lib.tk_fstats_plan_create(src, None, n, ctypes.byref(plan)) == INVALID
    assert lib.tk_fstats_plan_create(src, cnt, n, None) == INVALID
    assert lib.tk_fstats_plan_create(src, cnt, 0, ctypes.byref(plan)) == INVALID
    neg = (ctypes.c_int64 * 1)(-1)
    assert lib.tk_fstats_plan_create(src, neg, 1, ctypes.byref(plan)) == INVALID
    odd = (ctypes.c_void_p * 1)(ptrs[0] + 2)
    assert lib.tk_fstats_plan_create(odd, cnt, 1, ctypes.byref(plan)) == INVALID
    assert b"4-byte" in lib.tk_last_error()
    assert not plan.value
    assert lib.tk_float_range_reset(None, 1, _stream()) == INVALID
    assert lib.tk_float_range_reset(o, 0, _stream()) == INVALID
    assert lib.tk_float_range_batch(src, cnt, n, None, _stream()) == INVALID
    _ok(lib, lib.tk_fstats_plan_create(src, cnt, n, ctypes.byref(plan)))
    try:
        assert lib.tk_fstats_plan_range(plan, None, _stream()) == INVALID
        assert lib.tk_fstats_plan_range(None, o, _stream()) == INVALID
        for bins in (1, 0, -5, 8193):
            assert lib.tk_fstats_plan_histogram(plan, e, bins, o, _stream()) == INVALID
            assert lib.tk_float_histogram_batch(src, cnt, n, e, bins, o, _stream()) == INVALID
        assert lib.tk_fstats_plan_histogram(plan, None, 11, o, _stream()) == INVALID
        assert lib.tk_fstats_plan_histogram(plan, e, 11, None, _stream()) == INVALID
        for level in (-1, 3):
            assert lib.tk_fstats_plan_digits(plan, level, e, o, _stream()) == INVALID
            assert lib.tk_float_digits_batch(src, cnt, n, level, e, o, _stream()) == INVALID
        assert lib.tk_fstats_plan_digits(plan, 0, None, o, _stream()) == INVALID
        assert lib.tk_fstats_plan_digits(plan, 0, e, None, _stream()) == INVALID
    finally:
        lib.tk_fstats_plan_destroy(plan)
    assert lib.tk_fstats_plan_destroy(None) == 0


# ---------------------------------------------------------------- the module's accumulator

@pytest.fixture(scope="module")
def profile(device):
    """The float profile graph of a small ResNet-18, as collect_stats builds it, and two inputs."""
    m = zoo.resnet_float(18, batch=1, hw=32)
    mod = passes.annotate(passes.partition(passes.prerequisite_optimize(m.mod, m.params)))
    prof, _ = passes.stats_profile(mod)
    gm = graph_executor.GraphModule(relay.build(prof, target="mi355x")["default"]())
    yield gm, [{"data": m.random_input(seed=s)} for s in range(2)]
    gm.close()


def test_accumulator_against_host_copies(profile):
    gm, inputs = profile
    names = [t.name for t in gm.plan.records if str(t.dtype) == "float32"]
    acc = gm.float_stats_accumulator()
    assert acc.names == names and len(names) > 10
    some = gm.float_stats_accumulator(names[2::5])
    copies = {n: [] for n in names}
    for x in inputs:
        gm.run(**x)
        acc.add_range()
        some.add_range()
        for n in names:
            copies[n].append(gm.get_node_output(n).numpy().reshape(-1))
    whole = {n: np.concatenate(v) for n, v in copies.items()}
    ranges = acc.ranges()
    for n in names:
        r = ranges[n]
        assert (r.count, r.nonfinite, r.min, r.max) == (whole[n].size, 0, whole[n].min(), whole[n].max()), n
    assert some.ranges() == {n: ranges[n] for n in names[2::5]}
    acc.set_edges(8001)
    for x in inputs:
        gm.run(**x)
        acc.add_histogram()
    for n, (hist, edges) in acc.histograms().items():
        thres = max(abs(whole[n].min()), abs(whole[n].max()))
        want, want_edges = np.histogram(whole[n], bins=8001, range=(-thres, thres))
        assert np.array_equal(edges.view(np.uint32), want_edges.view(np.uint32)), n
        assert np.array_equal(hist, want.astype(np.uint64)), n

    def count(level, prefixes):
        for x in inputs:
            gm.run(**x)
            acc.add_digits(level, prefixes)
        tables = acc.digits()
        return [tables[n] for n in names]

    bits = passes.radix_select(count, lambda total: int(total * 0.99999))
    for n, b in zip(names, bits):
        assert np.array([b], np.uint32).view(np.float32)[0] == passes.find_scale_by_percentile(whole[n]), n
    acc.reset_ranges()
    assert all(r.count == 0 and r.min == np.inf for r in acc.ranges().values())


def test_float_stats_plan_names(profile, device):
    gm, _ = profile
    with pytest.raises(KeyError):
        gm.float_stats_accumulator(["no such record"])
    m = zoo.lenet5(batch=2)
    q = graph_executor.GraphModule(relay.build(m.mod, target="mi355x", params=m.params)["default"](None, tune=False))
    try:
        integer = next(t.name for t in q.plan.records if str(t.dtype) != "float32")
        with pytest.raises(ValueError):
            q.float_stats_accumulator([integer])
    finally:
        q.close()


def test_closed_module_refuses(device):
    m = zoo.resnet_float(18, batch=1, hw=32)
    mod = passes.annotate(passes.partition(passes.prerequisite_optimize(m.mod, m.params)))
    gm = graph_executor.GraphModule(relay.build(passes.stats_profile(mod)[0], target="mi355x")["default"]())
    acc = gm.float_stats_accumulator()
    gm.run(data=m.random_input())
    acc.add_range()
    assert sum(r.count for r in acc.ranges().values()) > 0
    gm.close()
    for call in (acc.add_range, acc.ranges, lambda: acc.set_edges(11), acc.add_histogram, acc.histograms,
                 lambda: acc.add_digits(0), acc.digits, acc.reset_ranges):
        with pytest.raises(_lib.TachikomaError):
            call()


# ---------------------------------------------------------------- end to end

@pytest.mark.parametrize("mode", ["kl_divergence", "percentile"])
def test_device_calibration_equals_host_calibration(device, mode, monkeypatch):
    """quantize(..., device_stats=True) binds the constants the host path binds, byte for byte,
    and reads no activation back."""
    m = zoo.resnet_float(18, batch=2, hw=64)
    data = [{"data": m.random_input(seed=s)} for s in range(2)]
    with qconfig(calibrate_mode=mode):
        q_host = quantize(m.mod, m.params, dataset=data)
    host_consts = [n.data for n in relay.post_order(q_host["main"].body) if isinstance(n, relay.Constant)]

    def no_readback(self, name):
        raise AssertionError(f"the device calibration read {name} back")

    runs = []
    run = graph_executor.GraphModule.run
    monkeypatch.setattr(graph_executor.GraphModule, "get_node_output", no_readback)
    monkeypatch.setattr(graph_executor.GraphModule, "run", lambda self, *a, **k: (runs.append(1), run(self, *a, **k))[1])
    with qconfig(calibrate_mode=mode, calibrate_chunk_by=3):
        q_dev = quantize(m.mod, m.params, dataset=data, device_stats=True)
    monkeypatch.undo()
    assert len(runs) == (2 if mode == "kl_divergence" else 3) * len(data)
    dev_consts = [n.data for n in relay.post_order(q_dev["main"].body) if isinstance(n, relay.Constant)]
    assert len(dev_consts) == len(host_consts) > 20
    for a, b in zip(dev_consts, host_consts):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_device_calibration_refuses_nonfinite_activations(device):
    """One infinite input element: each pixel of the first convolution sees it under one weight, so
    the output channels with a positive weight there carry +inf through the ReLU into a profiled
    record (a NaN would not do: the kernels' ReLU maps it to 0)."""
    m = zoo.resnet_float(18, batch=1, hw=32)
    x = m.random_input()
    x.reshape(-1)[5] = np.inf
    for mode in ("kl_divergence", "percentile"):
        with qconfig(calibrate_mode=mode):
            with pytest.raises(ValueError, match="NaN or infinite"):
                quantize(m.mod, m.params, dataset=[{"data": x}], device_stats=True)
