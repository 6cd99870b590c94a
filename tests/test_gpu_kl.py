"""The kl_divergence threshold search on the MI355X (csrc/tk_kl.hip) against the host's MinimizeKL
(tk_kl_candidates, tk_find_scale_by_kl) and the numpy model of tests/kl_cases.py: the exact parts
of the device table are equal to the host's, every host divergence lies within the device's bound,
the device's float64 divergence is the model's, the picks are the selection rule applied to the
table and contain the host's argmin, and kl_thresholds / quantize(device_kl=True) give the host
path's bytes.  Device calls take 5 records and 1 record."""
import ctypes

import numpy as np
import pytest

from tachikoma_amd import _lib, relay, zoo
from tachikoma_amd.contrib import graph_executor, trace_device
from tachikoma_amd.relay.quantize import passes, qconfig, quantize
from tests import kl_cases as kc

pytestmark = pytest.mark.gpu

INVALID = -1


@pytest.fixture(scope="module")
def lib(device):
    return _lib.load()


def _stream():
    return ctypes.c_void_p(_lib.stream_handle())


def _device_search(lib, device, hists, bins, buckets):
    """tk_kl_device over len(hists) records: (rows [n, n_cand], picks [n])."""
    import torch
    n, n_cand = len(hists), kc.n_candidates(bins, buckets)
    assert lib.tk_kl_row_size() == kc.ROW_DTYPE.itemsize and lib.tk_kl_pick_size() == kc.PICK_DTYPE.itemsize
    h = torch.from_numpy(np.stack(hists).astype(np.uint64).view(np.int64)).to(device)
    table = torch.full((n * n_cand * kc.ROW_DTYPE.itemsize // 8,), -1, dtype=torch.int64, device=device)
    picks = torch.full((n * kc.PICK_DTYPE.itemsize // 8,), -1, dtype=torch.int64, device=device)
    rc = lib.tk_kl_device(ctypes.c_void_p(h.data_ptr()), n, bins, buckets, ctypes.c_void_p(table.data_ptr()),
                          ctypes.c_void_p(picks.data_ptr()), _stream())
    assert rc == 0, lib.tk_last_error().decode()
    rows = table.cpu().numpy().view(kc.ROW_DTYPE).reshape(n, n_cand)
    return rows, picks.cpu().numpy().view(kc.PICK_DTYPE)


def _check_record(label, bins, buckets, hist, rows, pick):
    kind = label.split("-")[0]
    if hist.max() > kc.INT32_MAX:
        assert (int(pick["status"]), int(pick["count"])) == (kc.OVERFLOW, 0), label
        return
    host = kc.host_candidates(hist, bins, buckets)
    fin = np.isfinite(host["div"])
    # the exact parts are equal; +inf sits exactly where the host has it, with bound 0
    for field in ("ps", "qs", "p_zeros", "q_zeros"):
        assert np.array_equal(rows[field], host[field]), (label, field)
    assert np.array_equal(np.isinf(rows["d"]), ~fin), label
    assert np.all(rows["bound"][~fin] == 0), label
    err = np.abs(host["div"][fin].astype(np.float64) - rows["d"][fin])
    used = float((err / rows["bound"][fin]).max()) if fin.any() else 0.0
    print(f"{label}: largest |div_host - d| / bound = {used:.3f}")
    assert np.all(err <= rows["bound"][fin]), (label, used)
    # the select kernel is the selection rule over the device's own table
    status, keep = kc.survivors(hist, rows)
    assert (int(pick["status"]), int(pick["count"])) == (status, len(keep)), label
    assert list(pick["idx"][:min(len(keep), kc.K)]) == keep[:kc.K], label
    assert np.all(pick["idx"][len(keep):] == -1), label
    if (bins, buckets) in kc.FULL:
        assert status == kc.FULL_STATUS[kind], label
    if fin.any():
        assert kc.first_minimum(host["div"]) in keep, label
    # the float64 divergence is the model's but for the last place of a log (every candidate of the
    # small shapes; at full size a stride of them, the survivors and both ends)
    n = rows.size
    cand = np.arange(n) if n < 600 else np.unique(np.concatenate([np.arange(0, n, 97), [n - 1], keep[:kc.K]]).astype(int))
    want = kc.model(hist, bins, buckets, cand)
    got = rows[cand]
    assert np.array_equal(np.isinf(got["d"]), np.isinf(want["d"])), label
    f = np.isfinite(want["d"])
    assert np.all(np.abs(got["d"][f] - want["d"][f]) <= 1e-12 * np.abs(want["d"][f])), label
    assert np.all(np.abs(got["bound"][f] - want["bound"][f]) <= 1e-9 * want["bound"][f]), label


@pytest.mark.parametrize("bins,buckets", kc.SHAPES)
def test_table_and_picks(lib, device, bins, buckets):
    cases = kc.cases([(bins, buckets)])
    five, rest = cases[:5], cases[5:]
    rows, picks = _device_search(lib, device, [c[3] for c in five], bins, buckets)
    for i, (label, _, _, hist) in enumerate(five):
        _check_record(label, bins, buckets, hist, rows[i], picks[i])
    for label, _, _, hist in rest:
        rows, picks = _device_search(lib, device, [hist], bins, buckets)
        _check_record(label, bins, buckets, hist, rows[0], picks[0])


def test_refusals(lib, device):
    import torch
    buf = torch.zeros(4096, dtype=torch.int64, device=device)
    p = ctypes.c_void_p(buf.data_ptr())
    for bins, buckets in ((100, 11), (2, 2), (1, 2), (8193, 255), (101, 1), (101, 102)):
        assert lib.tk_kl_device(p, 1, bins, buckets, p, p, _stream()) == INVALID, (bins, buckets)
    assert lib.tk_kl_device(None, 1, 101, 11, p, p, _stream()) == INVALID
    assert lib.tk_kl_device(p, 1, 101, 11, None, p, _stream()) == INVALID
    assert lib.tk_kl_device(p, 1, 101, 11, p, None, _stream()) == INVALID
    assert lib.tk_kl_device(p, 0, 101, 11, p, p, _stream()) == INVALID


# ---------------------------------------------------------------- the accumulator

class _Plan:
    handle = None

    def __init__(self, names):
        self.names = names


def _accumulator(gm, cases, bins):
    """An accumulator of gm's module whose histograms are the cases' counts, loaded directly."""
    import torch
    names = [c[0] for c in cases]
    acc = trace_device.FloatStatsAccumulator(gm.module, _Plan(names))
    acc.bins = bins
    acc._edges_host = np.stack([kc.edges_of(bins) * np.float32(1 + i) for i in range(len(names))])
    acc._hist = torch.from_numpy(np.stack([c[3] for c in cases]).astype(np.uint64).view(np.int64).reshape(-1)).to(gm.module.device)
    return acc


@pytest.fixture(scope="module")
def small_module(device):
    m = zoo.lenet5(batch=2)
    gm = graph_executor.GraphModule(relay.build(m.mod, target="mi355x", params=m.params)["default"](None, tune=False))
    yield gm
    gm.close()


@pytest.mark.parametrize("bins,buckets", kc.SHAPES)
def test_kl_thresholds_equal_kl_threshold(small_module, bins, buckets):
    """Every case, the fallbacks included, as float32 bytes; an overflowing record raises."""
    cases = kc.cases([(bins, buckets)])
    ok = [c for c in cases if c[3].max() <= kc.INT32_MAX]
    acc = _accumulator(small_module, ok, bins)
    got = acc.kl_thresholds(buckets)
    statuses = set()
    for i, (label, _, _, hist) in enumerate(ok):
        want = passes.kl_threshold(hist, acc._edges_host[i], -1.0, "int8", bins, buckets)
        assert np.float32(got[label]).tobytes() == np.float32(want).tobytes(), label
        status = int(acc.kl_picks[i]["status"])
        statuses.add(status)
        assert (label in acc.kl_fallbacks) == (status != kc.OK), label
        if (bins, buckets) in kc.FULL:
            assert status == kc.FULL_STATUS[label.split("-")[0]], label
    assert kc.ALL_INF in statuses and kc.OK in statuses
    if (bins, buckets) in kc.FULL:
        assert kc.TOO_MANY in statuses
    table = acc.kl_table()
    assert set(table) == {c[0] for c in ok}
    assert all(t.dtype == trace_device.KL_ROW_DTYPE and t.size == kc.n_candidates(bins, buckets) for t in table.values())
    acc.close()
    bad = _accumulator(small_module, [c for c in cases if c[3].max() > kc.INT32_MAX][:1] + ok[:1], bins)
    with pytest.raises(ValueError, match="int32 counts"):
        bad.kl_thresholds(buckets)
    bad.close()


def test_kl_thresholds_misuse(small_module):
    acc = _accumulator(small_module, kc.cases([(101, 11)])[:2], 101)
    for buckets in (1, 102):
        with pytest.raises(ValueError):
            acc.kl_thresholds(buckets)
    with pytest.raises(ValueError):
        acc.kl_table()  # nothing searched yet
    acc.close()
    even = _accumulator(small_module, [("even", 100, 11, np.ones(100, np.int64))], 100)
    with pytest.raises(ValueError, match="odd"):
        even.kl_thresholds(11)
    even.close()
    fresh = trace_device.FloatStatsAccumulator(small_module.module, _Plan(["a"]))
    with pytest.raises(ValueError, match="set_edges"):
        fresh.kl_thresholds()
    fresh.close()


def test_closed_module_refuses_kl_thresholds(device):
    m = zoo.lenet5(batch=2)
    gm = graph_executor.GraphModule(relay.build(m.mod, target="mi355x", params=m.params)["default"](None, tune=False))
    acc = _accumulator(gm, kc.cases([(101, 11)])[:2], 101)
    assert len(acc.kl_thresholds(11)) == 2
    gm.close()
    for call in (lambda: acc.kl_thresholds(11), acc.kl_table):
        with pytest.raises(_lib.TachikomaError):
            call()


# ---------------------------------------------------------------- end to end

def test_device_kl_calibration_equals_host_calibration(device, monkeypatch):
    """quantize(..., device_stats=True, device_kl=True) binds the constants the host path binds,
    byte for byte, reads no record back and sends no layer through kl_threshold."""
    m = zoo.resnet_float(18, batch=2, hw=64)
    data = [{"data": m.random_input(seed=s)} for s in range(2)]
    with qconfig(calibrate_mode="kl_divergence"):
        q_host = quantize(m.mod, m.params, dataset=data)
    host_consts = [n.data for n in relay.post_order(q_host["main"].body) if isinstance(n, relay.Constant)]

    def no_readback(self, name):
        raise AssertionError(f"the device calibration read {name} back")

    runs, kl_calls, picks = [], [], []
    run = graph_executor.GraphModule.run
    kl_threshold = passes.kl_threshold
    search = trace_device.FloatStatsAccumulator.kl_thresholds

    def counted_search(self, *a, **k):
        out = search(self, *a, **k)
        picks.append(self.kl_picks.copy())
        return out

    monkeypatch.setattr(graph_executor.GraphModule, "get_node_output", no_readback)
    monkeypatch.setattr(graph_executor.GraphModule, "run", lambda self, *a, **k: (runs.append(1), run(self, *a, **k))[1])
    monkeypatch.setattr(passes, "kl_threshold", lambda *a, **k: (kl_calls.append(1), kl_threshold(*a, **k))[1])
    monkeypatch.setattr(trace_device.FloatStatsAccumulator, "kl_thresholds", counted_search)
    with qconfig(calibrate_mode="kl_divergence", calibrate_chunk_by=3):
        q_dev = quantize(m.mod, m.params, dataset=data, device_stats=True, device_kl=True)
    monkeypatch.undo()
    assert len(runs) == 2 * len(data)
    assert kl_calls == []
    assert len(picks) == 1 and picks[0].size > 10 and np.all(picks[0]["status"] == kc.OK)
    print("survivors per layer:", picks[0]["count"].tolist())
    dev_consts = [n.data for n in relay.post_order(q_dev["main"].body) if isinstance(n, relay.Constant)]
    assert len(dev_consts) == len(host_consts) > 20
    for a, b in zip(dev_consts, host_consts):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_device_kl_misuse_is_refused():
    m = zoo.resnet_float(18, batch=1, hw=32)
    data = [{"data": m.random_input()}]
    with qconfig(calibrate_mode="kl_divergence"):
        with pytest.raises(ValueError, match="device_stats"):
            quantize(m.mod, m.params, dataset=data, device_kl=True)
        mod = passes.annotate(passes.partition(passes.prerequisite_optimize(m.mod, m.params)))
        with pytest.raises(ValueError, match="device_stats"):
            passes.calibrate(mod, data, device_kl=True)
    for mode in ("percentile", "global_scale"):
        with qconfig(calibrate_mode=mode):
            with pytest.raises(ValueError, match="kl_divergence"):
                quantize(m.mod, m.params, dataset=data, device_stats=True, device_kl=True)
    with pytest.raises(ValueError, match="kl_divergence"):
        passes.device_scales(mod, data, "percentile", device_kl=True)
