"""Per-record statistics through the module layers on the MI355X: GraphModule.record_stats and
stats_accumulator against the host twin (trace_format.record_stats of each record's host copy),
statistics of loaded trace files against trace_format.trace_stats, the trace job's --stats
sidecars and --stats-only, and the teardown order of a module with a live accumulator.  All
results are integers: every check is equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tachikoma_amd import relay, trace_job, zoo
from tachikoma_amd import trace_format as tf
from tachikoma_amd.contrib import graph_executor
from tachikoma_amd.relay.quantize import quantize

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _zoo(name, **kw):
    def make():
        m = zoo.MODELS[name](**kw)
        lib = relay.build(m.mod, target="mi355x", params=m.params)
        batch = kw["batch"]
        return lib, [{m.input_name: m.sample_inputs(i * batch, batch)} for i in range(3)]
    return make


def _realized():
    """A realized float graph (its float32 records are the ones the kernel does not cover)."""
    m = zoo.resnet_float(18, batch=1, hw=32)
    lib = relay.build(quantize(m.mod, m.params), target="mi355x")
    x = m.random_input()
    return lib, [{"data": x}, {"data": np.ascontiguousarray(x[..., ::-1]) * np.float32(0.5)},
                 {"data": x * np.float32(0.25)}]


GRAPHS = {"lenet5": _zoo("lenet5", batch=3), "resnet18": _zoo("resnet18", batch=2, hw=32),
          "mobilenet_v2": _zoo("mobilenet_v2", batch=2, hw=32), "realized": _realized}


@pytest.fixture(scope="module", params=list(GRAPHS))
def graph(request, device):
    lib, inputs = GRAPHS[request.param]()
    gm = graph_executor.GraphModule(lib["default"]())
    yield request.param, lib, gm, inputs
    gm.close()


def _host_stats(gm, names):
    return {n: tf.record_stats(gm.get_node_output(n).numpy(), n) for n in names}


def _assert_equal(got, want):
    assert list(got) == list(want)
    for k in want:
        assert got[k].equals(want[k]) and got[k].name == k, (k, got[k], want[k])


def _split(gm):
    recs = [(t.name, str(t.dtype)) for t in gm.plan.records]
    return [n for n, d in recs if d in tf.STATS_KIND], [n for n, d in recs if d not in tf.STATS_KIND]


def test_record_stats_after_run(graph):
    name, _, gm, inputs = graph
    supported, unsupported = _split(gm)
    gm.run(**inputs[0])
    got = gm.record_stats()
    _assert_equal(got, _host_stats(gm, supported))
    assert all(s.count > 0 for s in got.values())
    acc = gm.stats_accumulator()
    assert acc.skipped == unsupported and acc.names == supported
    assert bool(unsupported) == (name == "realized")
    # the same buffers again: the one-shot form starts from the identity every time
    _assert_equal(gm.record_stats(), got)


def test_accumulator_over_three_inputs(graph):
    _, _, gm, inputs = graph
    supported, _ = _split(gm)
    acc = gm.stats_accumulator()
    some = supported[1::3]
    part = gm.stats_accumulator(names=some)
    singles = []
    for x in inputs:
        gm.run(**x)
        acc.add()
        part.add()
        singles.append(gm.record_stats())
    want = tf.merge_stats_dicts(singles)
    _assert_equal(acc.result(), want)
    _assert_equal(part.result(), {k: want[k] for k in some})
    assert acc.result()[supported[-1]].count == 3 * singles[0][supported[-1]].count
    acc.reset()
    assert all(s.equals(tf.RecordStats.empty(s.dtype)) for s in acc.result().values())
    with pytest.raises(KeyError):
        gm.stats_accumulator(names=["no such record"])


@pytest.mark.parametrize("packed", [False, True])
def test_statistics_of_a_loaded_trace(graph, tmp_path, packed):
    _, lib, gm, inputs = graph
    gm.run(**inputs[1])
    path = gm.dump_trace(str(tmp_path / "t.tkt"), packed=packed)
    want = tf.trace_stats(path)
    fresh = graph_executor.GraphModule(lib["default"](None, tune=False))
    try:
        fresh.load_trace(path)
        _assert_equal(fresh.record_stats(), want)
    finally:
        fresh.close()
    _assert_equal(gm.record_stats(), want)


def _job(tmp_path, name, *flags):
    d = str(tmp_path / name)
    assert trace_job.main(["--model", "lenet5", "--samples", "14", "--chunk", "4", "--out-dir", d, *flags]) == 0
    return d, trace_job.Journal(trace_job.journal_file(d, 0)).entries()


def test_trace_job_stats(device, tmp_path):
    plain, plain_entries = _job(tmp_path, "plain")
    assert len(plain_entries) == 4
    assert not [f for f in os.listdir(plain) if f.endswith(".stats.json")]
    merged = {}
    for flags in ((), ("--packed",)):
        d, entries = _job(tmp_path, "stats" + "".join(flags), "--stats", *flags)
        assert len(entries) == 4
        for i, e in entries.items():
            ref = plain_entries[i]
            assert e["digest"] == ref["digest"] and e["file"] == ref["file"] and e["n_samples"] == ref["n_samples"]
            if not flags:
                assert e == ref
        parts = []
        for e in entries.values():
            chunk = os.path.join(d, e["file"])
            side = trace_job.read_stats_file(trace_job.stats_file(chunk))
            want = tf.trace_stats(chunk)
            _assert_equal(side, want)
            parts.append(want)
        assert not [f for f in os.listdir(d) if f.endswith(".tmp")]
        merged[flags] = trace_job.read_stats_file(trace_job.rank_stats_file(d, 0))
        _assert_equal(merged[flags], tf.merge_stats_dicts(parts))
    _assert_equal(merged[("--packed",)], merged[()])
    only, _ = _job(tmp_path, "only", "--stats-only")
    assert sorted(os.listdir(only)) == ["trace.rank0.stats.json"]
    _assert_equal(trace_job.read_stats_file(trace_job.rank_stats_file(only, 0)), merged[()])


CHILD = """
import sys
sys.path.insert(0, {root!r})
from tachikoma_amd import _lib, relay, zoo
from tachikoma_amd.contrib import graph_executor
m = zoo.lenet5(batch=2)
lib = relay.build(m.mod, target="mi355x", params=m.params)
for order in ("module first", "accumulator first"):
    gm = graph_executor.GraphModule(lib["default"](None, tune=False))
    gm.run(**{{m.input_name: m.sample_inputs(0, 2)}})
    acc = gm.stats_accumulator()
    acc.add()
    n = sum(s.count for s in acc.result().values())
    acc.add()   # work in flight when the teardown starts
    if order == "module first":
        gm.close()
        try:
            acc.add()
        except _lib.TachikomaError:
            print("refused after close", flush=True)
        acc.close()
    else:
        acc.close()
        gm.close()
    print(order, n > 0, flush=True)
print("clean", flush=True)
"""


def test_teardown_with_a_live_accumulator(device):
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["refused", "after", "close", "module", "first", "True", "accumulator", "first", "True",
                                "clean"], r.stdout
