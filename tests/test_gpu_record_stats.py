"""The statistics kernel on the MI355X (csrc/tk_stats.hip) through its C ABI: tk_record_stats_batch
and the plan calls against plain numpy (tests/stats_cases.py).  All results are integers: every
check is equality.  Element counts sit on every edge of the kernel's geometry (a lane's 16 bytes,
the workgroup's 256 lanes, the tile T, the span S a workgroup walks before it flushes), sources at
every alignment the ABI allows, contents at both ends of the histogram contention (all one value,
uniform over the dtype)."""
import ctypes

import numpy as np
import pytest

from tachikoma_amd import _lib
from tachikoma_amd import trace_format as tf
from tests import stats_cases as sc

pytestmark = pytest.mark.gpu

OFFSETS = {0: (0, 4, 8, 12), 1: (0, 1, 2, 3, 15), 2: (0, 1, 2, 3, 15)}


@pytest.fixture(scope="module")
def lib(device):
    return _lib.load()


def _counts(lib):
    t, s = lib.tk_record_stats_tile(), lib.tk_record_stats_span()
    assert t > 257 and s % t == 0 and s > t
    return [1, 3, 4, 5, 15, 16, 17, 255, 256, 257, t - 1, t, t + 1, 2 * t + 3, s - 1, s + 1, 2 * s + 5]


class Arena:
    """Records laid out in one device buffer, each at its own offset from a 64-byte-aligned base."""

    def __init__(self):
        self.parts, self.at, self.size = [], [], 0

    def add(self, x, offset=0):
        raw = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
        start = self.size + offset
        self.parts.append((start, raw))
        self.at.append(start)
        self.size = (start + raw.size + 63) // 64 * 64 + 64
        return len(self.at) - 1

    def upload(self, device):
        import torch
        host = np.zeros(max(64, self.size), np.uint8)
        for start, raw in self.parts:
            host[start:start + raw.size] = raw
        self.dev = torch.from_numpy(host).to(device)
        assert self.dev.data_ptr() % 64 == 0
        return [self.dev.data_ptr() + a for a in self.at]


def _args(ptrs, counts, kinds):
    n = len(ptrs)
    return ((ctypes.c_void_p * max(1, n))(*ptrs), (ctypes.c_int64 * max(1, n))(*counts),
            (ctypes.c_int32 * max(1, n))(*kinds), n)


def _batch(lib, ptrs, counts, kinds):
    src, cnt, kd, n = _args(ptrs, counts, kinds)
    out = np.zeros(n, tf.STATS_DTYPE)
    rc = lib.tk_record_stats_batch(src, cnt, kd, n, ctypes.c_void_p(out.ctypes.data),
                                   ctypes.c_void_p(_lib.stream_handle()))
    assert rc == 0, lib.tk_last_error().decode()
    return out


def _check(rows, arrays, labels):
    for row, x, label in zip(rows, arrays, labels):
        sc.assert_is(tf.RecordStats.from_struct(row, str(x.dtype)), x, label)


def test_struct_size(lib):
    assert ctypes.sizeof(_lib.tk_record_stats) == lib.tk_record_stats_size() == tf.STATS_DTYPE.itemsize


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_counts_offsets_contents(lib, device, kind):
    rng = np.random.default_rng(100 + kind)
    arena, arrays, labels = Arena(), [], []
    for n in _counts(lib):
        for off in OFFSETS[kind]:
            for what, x in sc.contents(kind, n, rng).items():
                arena.add(x, off)
                arrays.append(x)
                labels.append((n, off, what))
    ptrs = arena.upload(device)
    rows = _batch(lib, ptrs, [a.size for a in arrays], [kind] * len(arrays))
    _check(rows, arrays, labels)
    # integer merges commute: a second run gives the same bytes
    again = _batch(lib, ptrs, [a.size for a in arrays], [kind] * len(arrays))
    assert rows.tobytes() == again.tobytes()


def test_mixed_batch_of_300(lib, device):
    rng = np.random.default_rng(5)
    t = lib.tk_record_stats_tile()
    arena, arrays, kinds = Arena(), [], []
    for i in range(300):
        kind = int(rng.integers(0, 3))
        n = 0 if i % 37 == 5 else (3 * t + 1 if i == 123 else int(rng.integers(1, 3 * t + 1)))
        x = list(sc.contents(kind, n, rng).values())[i % 5]
        arena.add(x, 0 if kind == 0 else int(rng.integers(0, 16)))
        arrays.append(x)
        kinds.append(kind)
    assert sum(a.size == 0 for a in arrays) >= 5 and max(a.size for a in arrays) == 3 * t + 1
    ptrs = arena.upload(device)
    rows = _batch(lib, ptrs, [a.size for a in arrays], kinds)
    _check(rows, arrays, list(range(300)))
    for row, x in zip(rows, arrays):
        if x.size == 0:
            assert (row["count"], row["sum"], row["min"], row["max"]) == (0, 0, sc.I32_MAX, sc.I32_MIN)
            assert not row["bits"].any() and not row["values"].any()


def test_record_of_more_than_512_spans(lib, device):
    """All workgroups of a record flush into one entry, so a record of more than 512 spans is cut
    into 512 longer runs: one record just past that threshold, one of exactly 512 spans beside it."""
    rng = np.random.default_rng(6)
    s = lib.tk_record_stats_span()
    big = rng.integers(0, 256, 514 * s + 12345, dtype=np.uint8)
    big[rng.random(big.size) < 0.9] = 0
    big[0], big[-1] = 255, 254
    edge = rng.integers(-3, 4, 512 * s).astype(np.int8)
    wide = sc.contents(0, 3 * s + 1, rng)["extremes"]
    arrays = [big, edge, wide, big[:513 * s - 7]]
    arena = Arena()
    for x, off in zip(arrays, (0, 0, 0, 3)):
        arena.add(x, off)
    ptrs = arena.upload(device)
    rows = _batch(lib, ptrs, [a.size for a in arrays], [2, 1, 0, 2])
    _check(rows, arrays, ["past 512 spans", "512 spans", "beside them", "past 512 spans, unaligned"])


class Plan:
    def __init__(self, lib, ptrs, counts, kinds):
        self.lib, self.handle = lib, ctypes.c_void_p()
        src, cnt, kd, n = _args(ptrs, counts, kinds)
        rc = lib.tk_stats_plan_create(src, cnt, kd, n, ctypes.byref(self.handle))
        assert rc == 0, lib.tk_last_error().decode()

    def run(self, stats):
        rc = self.lib.tk_stats_plan_run(self.handle, ctypes.c_void_p(stats.data_ptr()),
                                        ctypes.c_void_p(_lib.stream_handle()))
        assert rc == 0, self.lib.tk_last_error().decode()

    def close(self):
        assert self.lib.tk_stats_plan_destroy(self.handle) == 0


def _stats_array(device, n):
    import torch
    return torch.zeros(n * tf.STATS_DTYPE.itemsize // 8, dtype=torch.int64, device=device)


def _reset(lib, stats, n):
    assert lib.tk_record_stats_reset(ctypes.c_void_p(stats.data_ptr()), n, ctypes.c_void_p(_lib.stream_handle())) == 0


def _rows(stats):
    return stats.cpu().numpy().view(tf.STATS_DTYPE)


def _identity(rows):
    return all((r["count"], r["sum"], r["min"], r["max"]) == (0, 0, sc.I32_MAX, sc.I32_MIN) and
               not r["bits"].any() and not r["values"].any() for r in rows)


def test_plan_accumulates_over_runs(lib, device):
    import torch
    rng = np.random.default_rng(9)
    t, s = lib.tk_record_stats_tile(), lib.tk_record_stats_span()
    shapes = [(0, 2 * t + 3), (1, s + 1), (2, 777), (0, 0), (1, 5)]
    bufs = [torch.zeros(max(1, n), dtype=getattr(torch, np.dtype(sc.DTYPE[k]).name), device=device) for k, n in shapes]
    plan = Plan(lib, [b.data_ptr() for b in bufs], [n for _, n in shapes], [k for k, _ in shapes])
    stats = _stats_array(device, len(shapes))
    _reset(lib, stats, len(shapes))
    assert _identity(_rows(stats))
    seen = [[] for _ in shapes]
    for step in range(3):
        for i, (k, n) in enumerate(shapes):
            x = list(sc.contents(k, n, rng).values())[(step + i) % 5]
            seen[i].append(x)
            if n:
                bufs[i][:n].copy_(torch.from_numpy(x))
        plan.run(stats)
    rows = _rows(stats)
    for i, (k, n) in enumerate(shapes):
        got = tf.RecordStats.from_struct(rows[i], np.dtype(sc.DTYPE[k]).name)
        sc.assert_fields(got, sc.ref_merged(seen[i]), sc.DTYPE[k], i)
        assert got.count == 3 * n
    _reset(lib, stats, len(shapes))
    assert _identity(_rows(stats))
    plan.close()


def test_two_plans_share_one_stats_array(lib, device):
    rng = np.random.default_rng(10)
    t = lib.tk_record_stats_tile()
    xs = [sc.contents(0, t + 9, rng)["extremes"], sc.contents(1, 300, rng)["sparse"],
          sc.contents(2, 2 * t, rng)["extremes"], sc.contents(1, 17, rng)["small"]]
    arena = Arena()
    for x in xs:
        arena.add(x)
    ptrs = arena.upload(device)
    kinds = [0, 1, 2, 1]
    even = Plan(lib, ptrs, [xs[0].size, 0, xs[2].size, 0], kinds)   # entries 0 and 2; 1 and 3 are empty records
    odd = Plan(lib, ptrs, [0, xs[1].size, 0, xs[3].size], kinds)
    stats = _stats_array(device, 4)
    _reset(lib, stats, 4)
    even.run(stats)
    rows = _rows(stats)
    assert _identity([rows[1], rows[3]])
    odd.run(stats)
    _check(_rows(stats), xs, list(range(4)))
    even.close()
    odd.close()


def test_refusals_launch_nothing(lib, device):
    import torch
    buf = torch.zeros(64, dtype=torch.int32, device=device)
    p = buf.data_ptr()
    out = np.zeros(2, tf.STATS_DTYPE)
    outp = ctypes.c_void_p(out.ctypes.data)
    stream = ctypes.c_void_p(_lib.stream_handle())
    src, cnt, kd, n = _args([p, p], [8, 8], [0, 1])
    INVALID, UNSUPPORTED = -1, -2
    assert lib.tk_record_stats_batch(None, cnt, kd, n, outp, stream) == INVALID
    assert lib.tk_record_stats_batch(src, None, kd, n, outp, stream) == INVALID
    assert lib.tk_record_stats_batch(src, cnt, None, n, outp, stream) == INVALID
    assert lib.tk_record_stats_batch(src, cnt, kd, n, None, stream) == INVALID
    assert lib.tk_record_stats_batch(src, cnt, kd, 0, outp, stream) == INVALID
    null_src = _args([p, None], [8, 8], [0, 1])[0]
    assert lib.tk_record_stats_batch(null_src, cnt, kd, n, outp, stream) == INVALID
    assert lib.tk_record_stats_batch(src, cnt, _args([p, p], [8, 8], [0, 3])[2], n, outp, stream) == UNSUPPORTED
    assert lib.tk_record_stats_batch(src, cnt, _args([p, p], [8, 8], [-1, 1])[2], n, outp, stream) == UNSUPPORTED
    assert lib.tk_record_stats_batch(src, _args([p, p], [8, -1], [0, 1])[1], kd, n, outp, stream) == INVALID
    assert lib.tk_record_stats_batch(_args([p + 2, p], [8, 8], [0, 1])[0], cnt, kd, n, outp, stream) == INVALID
    assert b"tk_stats_plan_create" in lib.tk_last_error()
    handle = ctypes.c_void_p()
    assert lib.tk_stats_plan_create(src, cnt, kd, n, None) == INVALID
    assert lib.tk_stats_plan_create(src, cnt, kd, -3, ctypes.byref(handle)) == INVALID and not handle.value
    assert lib.tk_stats_plan_run(None, ctypes.c_void_p(p), stream) == INVALID
    assert lib.tk_record_stats_reset(None, 2, stream) == INVALID
    assert lib.tk_record_stats_reset(ctypes.c_void_p(p), 0, stream) == INVALID
    assert not out.view(np.uint8).any()   # nothing was written
    # a 1-byte record at the same odd address is fine
    rows = _batch(lib, [p + 2], [9], [1])
    assert rows[0]["count"] == 9 and rows[0]["values"][128] == 9
