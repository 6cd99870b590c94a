"""GraphModule.replay_trace on the MI355X: every op of a trace file re-executed from its recorded
inputs (records stored, shadows rebuilt in one launch, nodes run in reverse: relay/replay.py), so
that a fault stays in its node; load_trace(shadows=True), tk_module_run_order and
trace_job --check --replay.

Every test dumps the trace of input A and then runs the module on another input B before it
replays: a buffer the replay fails to rebuild from the file is then wrong, not accidentally right."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest

from tachikoma_amd import _lib, relay, trace_job, zoo
from tachikoma_amd import trace_format as tf
from tachikoma_amd.contrib import graph_executor
from tachikoma_amd.relay.contrib import tachikoma as tkbyoc
from tachikoma_amd.relay.quantize import quantize
from tachikoma_amd.relay.replay import replay_units

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- graphs
def _pad24():
    """Batch 3, 9x9 planes, 24 channels (padded shadow channels, unaligned planes): a conv block,
    two conv blocks on it joined by a qadd, two conv blocks, a max pool, a dense block."""
    shape = (3, 24, 9, 9)
    b = zoo._Builder(21)
    x = zoo._input(b, shape)
    x = zoo.conv_block(b, x, "c0", 24, 3, pad=1)
    p = zoo.conv_block(b, x, "p", 24, 3, pad=1, act=None)
    q = zoo.conv_block(b, x, "q", 24, 1, act=None)
    x = zoo.qadd(b, p, q, relu=True)
    x = zoo.conv_block(b, x, "c3", 24, 3, pad=1)
    x = zoo.conv_block(b, x, "c4", 24, 1)
    x = zoo.QTensor(relay.nn.max_pool2d(x.expr, pool_size=(2, 2), strides=(2, 2)), x.scale, x.zp, x.sigma)
    x = zoo.QTensor(relay.nn.batch_flatten(x.expr), x.scale, x.zp, x.sigma)
    x = zoo.dense_block(b, x, "fc", 10, act=None)
    return zoo._finish("pad24", b, x, shape, 21)


def _qnn(model, batch):
    lib = relay.build(model.mod, target="mi355x", params=model.params)
    return (graph_executor.GraphModule(lib["default"]()), {model.input_name: model.sample_inputs(0, batch)},
            {model.input_name: model.sample_inputs(batch, batch)})


def _realized():
    m = zoo.resnet_float(18, batch=1, hw=32)
    lib = relay.build(quantize(m.mod, m.params), target="mi355x")
    x = m.random_input()
    return (graph_executor.GraphModule(lib["default"]()), {"data": x},
            {"data": np.ascontiguousarray(x[..., ::-1]) * np.float32(0.5)})


NHWC_TEXT = """#[version = "0.0.5"]
def @main(%x: Tensor[(2, 9, 9, 16), float32], %w: Tensor[(3, 3, 16, 32), int8], %b: Tensor[(32), int32],
          %y: Tensor[(2, 9, 9, 8), int8]) {
  %0 = qnn.quantize(%x, 0.05f, -3, out_dtype="int8");
  %1 = qnn.conv2d(%0, %w, -3, 0, 0.05f, 0.02f, padding=[1, 1, 1, 1], channels=32, kernel_size=[3, 3],
                  data_layout="NHWC", kernel_layout="HWIO", out_dtype="int32");
  %2 = nn.bias_add(%1, %b, axis=3);
  %3 = qnn.requantize(%2, 0.001f, 0, 0.1f, 2, axis=3, out_dtype="int8");
  %4 = clip(%3, a_min=-128f, a_max=127f);
  %5 = (%4, %y);
  %6 = qnn.concatenate(%5, (0.1f, 0.07f), (2, -1), 0.09f, 1, axis=3);
  qnn.dequantize(%6, 0.09f, 1)
}
"""


def _nhwc():
    mod = relay.parse(NHWC_TEXT)
    rng = np.random.default_rng(3)
    params = {"w": rng.integers(-128, 128, (3, 3, 16, 32)).astype(np.int8),
              "b": rng.integers(-5000, 5000, 32).astype(np.int32)}

    def inputs():
        return {"x": rng.standard_normal((2, 9, 9, 16)).astype(np.float32) * 3,
                "y": rng.integers(-128, 128, (2, 9, 9, 8)).astype(np.int8)}

    lib = relay.build(mod, target="mi355x", params=params)
    return graph_executor.GraphModule(lib["default"]()), inputs(), inputs()


def _composite():
    from tests.test_tachikoma_byoc import conv_model
    mod, params, a = conv_model("MFMA")
    part = tkbyoc.partition_for_tachikoma(mod, params)
    rng = np.random.default_rng(9)
    b = {"data": rng.integers(0, 21, size=a["data"].shape).astype(np.uint8),
         "sum_in": rng.integers(0, 11, size=a["sum_in"].shape).astype(np.uint8)}
    lib = relay.build(part, target="mi355x", params=params)
    return graph_executor.GraphModule(lib["default"]()), a, b


CASES = {
    "lenet5_b3": lambda: _qnn(zoo.lenet5(batch=3), 3),
    "resnet18": lambda: _qnn(zoo.resnet18(batch=2, hw=32), 2),
    "resnet50": lambda: _qnn(zoo.resnet50(batch=2, hw=32), 2),
    "mobilenet_v2": lambda: _qnn(zoo.mobilenet_v2(batch=2, hw=32), 2),
    "pad24": lambda: _qnn(_pad24(), 3),
    "realized_resnet18": _realized,
    "nhwc_hwio": _nhwc,
    "composite": _composite,
}


@pytest.fixture(scope="module")
def graphs():
    """Built once per file (with the clean trace of input A, plain and packed, in memory), closed
    when the file is done."""
    import tempfile
    built = {}

    def get(which):
        if which not in built:
            gm, a, b = CASES[which]()
            gm.set_input(**a)
            with tempfile.TemporaryDirectory() as d:
                p1, p2 = os.path.join(d, "a.plain.tkt"), os.path.join(d, "a.packed.tkt")
                gm.dump_trace(p1)
                gm.dump_trace(p2, packed=True)
                files = (open(p1, "rb").read(), open(p2, "rb").read())
            assert tf.pack_trace(files[0]) == files[1]
            built[which] = (gm, a, b, files)
        return built[which]

    yield get
    for gm, *_ in built.values():
        gm.close()
    import gc
    gc.collect()


def _run_b(gm, b):
    """Another input through the module: every record, shadow and scratch buffer now holds B's."""
    gm.set_input(**b)
    gm.run()


def _record_shadows(gm):
    """Number of shadows whose source tensor is a record or a graph input."""
    recs = {t.name for t in gm.plan.records} | {t.name for t in gm.plan.inputs}
    return len({s for io in gm.module.node_io for s, src in io["shadows"].items() if src in recs})


def _node_of(gm):
    return {r: i for i, recs in enumerate(gm.module.node_records) for r in recs}


def _patched(plain, gm, changes):
    """The version-1 file with one element of each record in ``changes`` ({name: flat index})
    changed on the host, and the packed file pack_trace derives from it: ((plain, packed),
    {name: (new, old)})."""
    records = [(t.name, t.shape, t.dtype) for t in gm.plan.records]
    blob = bytearray(plain)
    ct = tf.check_trace(bytes(blob), records)
    values = {}
    for name, flat in changes.items():
        e = next(e for e in ct.entries if e.name == name)
        dt = np.dtype(e.dtype)
        at = ct.records_off + e.raw_off + flat * dt.itemsize
        old = np.frombuffer(bytes(blob[at:at + dt.itemsize]), dt)[0]
        new = dt.type(old + 1.5) if dt.kind == "f" else dt.type(old - 1 if old == np.iinfo(dt).max else old + 1)
        assert new != old
        blob[at:at + dt.itemsize] = np.array([new], dt).tobytes()
        values[name] = (new, old)
    return (bytes(blob), tf.pack_trace(bytes(blob))), values


# ---------------------------------------------------------------- clean files
@pytest.mark.parametrize("which", sorted(CASES))
def test_replay_clean(device, tmp_path, graphs, which):
    gm, a, b, files = graphs(which)
    path = str(tmp_path / "a.tkt")
    for blob in files:
        _run_b(gm, b)
        assert not gm.verify_trace(blob, run=False).ok          # the buffers hold B's records
        rep = gm.replay_trace(blob)                              # bytes
        assert rep.ok and rep.mismatches == [] and rep.nodes == [] and rep.first is None, (which, rep)
        assert rep.params_equal and rep.params_differing == []
        assert rep.n_records == len(gm.plan.records) == gm.verify_trace(blob).n_records
        assert rep.stats["shadows"] == _record_shadows(gm)
        assert all(rep.stats[k] >= 0 for k in ("store_ms", "shadow_ms", "replay_ms", "compare_ms"))
        _run_b(gm, b)
        open(path, "wb").write(blob)
        assert gm.replay_trace(path).ok                          # a path
    assert isinstance(rep, graph_executor.VerifyReport)
    if which in ("resnet18", "resnet50", "mobilenet_v2", "pad24"):
        assert _record_shadows(gm) > 0


def test_replay_refuses_a_damaged_file(device, graphs):
    gm, a, b, files = graphs("lenet5_b3")
    uploads = gm.trace_verifier().uploads
    with pytest.raises(ValueError):
        gm.replay_trace(files[1][:-100])
    assert gm.trace_verifier().uploads == uploads                # the device saw nothing


# ---------------------------------------------------------------- a fault in the engine
@pytest.mark.parametrize("which", ["lenet5_b3", "resnet18", "pad24"])
def test_engine_fault_stays_in_its_node(device, graphs, which):
    gm, a, b, files = graphs(which)
    convs = [o for o in gm.plan.ops if o.op == "qnn.conv2d"]
    conv = convs[len(convs) // 2]
    wname = conv.inputs[1]
    node = _node_of(gm)[conv.name]
    w = gm.module.buffers[wname].cpu().numpy()
    changed = w.copy()
    # one weight of output channel 0, moved by half its range (enough to pass the node's requantize
    # and show downstream): the centre tap of the input channel that most often differs from the
    # zero point where that tap reads it (after a ReLU much of a small plane IS the zero point,
    # and a weight that only ever meets zeros changes nothing)
    x = tf.read_trace(files[0]).records[conv.inputs[0]]
    (sh, sw), pad = conv.attrs["strides"], conv.attrs["padding"]
    r, s = w.shape[2] // 2, w.shape[3] // 2
    oh, ow = gm.plan.tensor(conv.name).shape[2:]
    iy, ix = np.arange(oh) * sh - pad[0] + r, np.arange(ow) * sw - pad[1] + s
    iy, ix = iy[(iy >= 0) & (iy < x.shape[2])], ix[(ix >= 0) & (ix < x.shape[3])]
    seen = (x[:, :, iy][:, :, :, ix] != conv.attrs["input_zero_point"]).sum(axis=(0, 2, 3))
    c = int(np.argmax(seen))
    assert seen[c] > 0
    w0 = int(w[0, c, r, s])
    changed[0, c, r, s] = w0 - 128 if w0 >= 0 else w0 + 128
    gm.set_input(wname, changed)
    try:
        for blob in files:
            ver = gm.verify_trace(blob)
            assert not ver.ok and ver.params_differing == [wname] and ver.first.name == conv.name
            _run_b(gm, b)
            rep = gm.replay_trace(blob)
            assert not rep.ok and rep.params_differing == [wname]
            assert rep.first is not None and rep.first.name == conv.name and rep.first.op == "qnn.conv2d"
            assert len(rep.nodes) == 1 and rep.nodes[0].node == node and rep.nodes[0].first == conv.name
            assert rep.nodes[0].records == tuple(gm.module.node_records[node])
            assert rep.nodes[0].kind == gm.module.node_kinds[node]
            got, all_ = {m.name for m in rep.mismatches}, {m.name for m in ver.mismatches}
            assert got <= set(gm.module.node_records[node]) and all(m.node == node for m in rep.mismatches)
            assert got < all_, (got, all_)                       # verify_trace also lists what lies downstream
    finally:
        gm.set_input(wname, w)
    assert gm.verify_trace(files[1]).ok


# ---------------------------------------------------------------- two faults in the file
@pytest.mark.parametrize("which", ["resnet18", "pad24"])
def test_two_independent_faults_are_both_found(device, graphs, which):
    gm, a, b, files = graphs(which)
    ops = gm.plan.ops
    feeds_conv = [o.name for o in ops if o.op == "clip" and
                  any(c.op == "qnn.conv2d" and c.inputs[0] == o.name for c in ops)]
    r1, r2 = feeds_conv[0], feeds_conv[-1]
    node_of = _node_of(gm)
    assert node_of[r1] < node_of[r2]
    # independent: the node that writes r2 does not read r1
    assert all(r1 not in o.inputs for o in ops if node_of[o.name] == node_of[r2])
    shapes = {t.name: t.shape for t in gm.plan.records}
    flat = {r: tf._n_elems(shapes[r]) * 2 // 3 for r in (r1, r2)}
    bad, values = _patched(files[0], gm, flat)
    # where a mismatch may show: the two records, and the records of the nodes that read them
    allowed = {r1, r2}
    for o in ops:
        if r1 in o.inputs or r2 in o.inputs:
            allowed |= set(gm.module.node_records[node_of[o.name]])
    for blob in bad:
        _run_b(gm, b)
        rep = gm.replay_trace(blob)
        assert not rep.ok and rep.params_equal
        by_name = {m.name: m for m in rep.mismatches}
        assert set(by_name) <= allowed, sorted(set(by_name) - allowed)
        for r in (r1, r2):
            m = by_name[r]
            assert (m.count, m.flat_index, m.node) == (1, flat[r], node_of[r]), m
            assert m.first_index == tuple(int(i) for i in np.unravel_index(flat[r], shapes[r]))
        faulty = {n.node for n in rep.nodes}
        assert node_of[r1] in faulty and node_of[r2] in faulty
        assert [n.node for n in rep.nodes] == sorted(faulty) and rep.first.node == rep.nodes[0].node
        expected, got = rep.detail(by_name[r1])                  # the file's changed value, the recomputed original
        assert (expected, got) == (values[r1][0], values[r1][1])
        # end to end, the second fault hides behind the first one's wake
        ver = gm.verify_trace(blob)
        assert ver.first.name == r1 and len(ver.mismatches) >= 2


# ---------------------------------------------------------------- afterwards
@pytest.mark.parametrize("which", ["resnet18", "nhwc_hwio"])
def test_module_is_intact_after_a_replay(device, graphs, which):
    gm, a, b, files = graphs(which)
    _run_b(gm, b)
    assert gm.replay_trace(files[1]).ok
    gm.set_input(**a)
    gm.run()
    assert gm.verify_trace(files[0], run=False).ok
    assert gm.verify_trace(files[1]).ok


@pytest.mark.parametrize("which", ["resnet18", "resnet50"])
def test_load_trace_with_shadows_then_run_range(device, graphs, which):
    gm, a, b, files = graphs(which)
    mod = gm.module
    units, upfront = replay_units(mod.node_io, [t.name for t in gm.plan.inputs])
    # conv blocks that read a record's shadow (the MFMA path): the one in the middle
    mfma = [u for u in units if mod.node_kinds[u[-1]] == "conv_block" and
            any(x in upfront for x in mod.node_io[u[-1]]["reads"])]
    unit = mfma[len(mfma) // 2]
    want = tf.read_trace(files[0]).records
    _run_b(gm, b)
    gm.load_trace(files[1], shadows=True)
    mod.run_range(unit[0], unit[-1] + 1)
    for name in mod.node_records[unit[-1]]:
        assert np.array_equal(gm.get_node_output(name).numpy(), want[name]), name


def test_run_order_refusals(device, graphs):
    gm, a, b, files = graphs("lenet5_b3")
    lib, mod = gm.module.lib, gm.module
    s = ctypes.c_void_p(_lib.stream_handle(None))
    I32 = ctypes.c_int32
    assert lib.tk_module_run_order(mod.handle, (I32 * 2)(0, mod.n_nodes), 2, s) == -1    # out of range
    assert b"out of range" in lib.tk_last_error()
    assert lib.tk_module_run_order(mod.handle, (I32 * 1)(-1), 1, s) == -1
    assert lib.tk_module_run_order(mod.handle, None, 1, s) == -1                         # null order, n > 0
    assert lib.tk_module_run_order(None, (I32 * 1)(0), 1, s) == -1
    assert lib.tk_module_run_order(mod.handle, None, 0, s) == 0
    with pytest.raises(_lib.TachikomaError):
        mod.run_order([mod.n_nodes])
    # the nodes in forward order are a run
    gm.set_input(**a)
    mod.run_order(list(range(mod.n_nodes)))
    assert gm.verify_trace(files[0], run=False).ok


# ---------------------------------------------------------------- trace job
@pytest.mark.parametrize("packed", [False, True])
def test_trace_job_check_replay(device, tmp_path, packed, capsys):
    d = str(tmp_path / "job")
    argv = ["--model", "lenet5", "--samples", "4", "--chunk", "2", "--out-dir", d]
    assert trace_job.main(argv + (["--packed"] if packed else [])) == 0
    capsys.readouterr()
    assert trace_job.main(argv + ["--check", "--replay"]) == 0
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert [r["chunk"] for r in lines] == [0, 1] and all(r["ok"] and r["nodes"] == [] for r in lines)
    assert all(r["packed"] is packed and r["shadows"] >= 0 and "replay_ms" in r for r in lines)
    # one record of chunk 1 changed: an int32 conv output in the middle of a fused node
    path = trace_job.chunk_file(d, 0, 1)
    plain = bytes(tf.unpack_trace(path)) if packed else open(path, "rb").read()
    trace = tf.read_trace(plain)
    names = list(trace.records)
    name = [k for k in names if trace.records[k].dtype == np.int32][-1]
    ct = tf.check_trace(plain, [(k, v.shape, str(v.dtype)) for k, v in trace.records.items()])
    e = next(e for e in ct.entries if e.name == name)
    blob = bytearray(plain)
    blob[ct.records_off + e.raw_off + 5 * 4] ^= 0x01             # element 5, its lowest bit
    src = str(tmp_path / "mod.tkt")
    open(src, "wb").write(tf.pack_trace(bytes(blob)) if packed else bytes(blob))
    shutil.copyfile(src, path)
    assert trace_job.main(argv + ["--check", "--replay"]) == 1
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert [r["ok"] for r in lines] == [True, False]
    assert lines[1]["first"]["name"] == name and lines[1]["n_mismatched"] >= 1
    nodes = lines[1]["nodes"]
    assert len(nodes) == 1 and name in nodes[0]["records"] and nodes[0]["first"] == name
    assert isinstance(nodes[0]["node"], int) and nodes[0]["kind"]
    with pytest.raises(SystemExit):                              # --replay is a mode of --check
        trace_job.main(argv + ["--replay"])
