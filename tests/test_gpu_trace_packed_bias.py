"""Packed trace files of version 3 on the MI355X: the deterministic packer with addends
(tk_wire_pack_device_bias) byte for byte against the host encoder, the device decoder with addends
(tk_wire_unpack_device_bias) in store and compare mode over the grid of the shared bias cases, and
the layers above them: dump_trace(packed=True, bias=True) against pack_trace(bias=True),
verify_trace / replay_trace / load_trace on version-3 files, and the trace job."""
import ctypes
import json

import numpy as np
import pytest

from tachikoma_amd import _lib, relay, trace_job, zoo
from tachikoma_amd import trace_format as tf
from tachikoma_amd.contrib import graph_executor
from tachikoma_amd.relay import qnn
from tests import wire_cases as wc
from tests import wire_cases_bias as wb

pytestmark = pytest.mark.gpu

NAMES = sorted(wb.cases(np.random.default_rng(0)))
FILL, GUARD = 0xA5, 32
NONE = (0, 0xFFFFFFFFFFFFFFFF)
STORE, COMPARE = _lib.TK_WIRE_UNPACK_STORE, _lib.TK_WIRE_UNPACK_COMPARE


@pytest.fixture(scope="module", autouse=True)
def _collect_after():
    yield
    import gc
    gc.collect()


@pytest.fixture(scope="module")
def cases():
    """The shared cases, once: name -> (records, diffs, addends, flat)."""
    return wb.cases(np.random.default_rng(7))


def _host_wire(records, diffs, addends):
    lib = _lib.load()
    offs, total = wc.layout(records)
    recs, ads = wb.wire_records(records, diffs, addends, offs)
    src = wc.image_of(records, offs, total)
    bound = lib.tk_wire_bound(recs, len(records))
    assert bound > 0, lib.tk_last_error()
    wire = np.full(bound, 0x11, np.uint8)
    used = lib.tk_wire_encode_host_bias(recs, ads, len(records), wc.ptr(src), total, wc.ptr(wire), bound)
    assert used > 0, lib.tk_last_error()
    return bound, wire[:used].copy()


def _device_addends(records, diffs, addends):
    """(records, addend array with device pointers, the tensors that keep them alive)."""
    import torch
    keep = {i: torch.from_numpy(ad[2].copy()).cuda() for i, ad in enumerate(addends) if ad is not None}
    recs, ads = wb.wire_records(records, diffs, addends, [0] * len(records), {i: t.data_ptr() for i, t in keep.items()})
    return recs, ads, keep


def _pack(recs, ads, n, ptrs, bound):
    """(used, the whole buffer), pre-filled: a byte the packer leaves unwritten inside [0, used)
    differs from the host encoder's zero."""
    import torch
    lib = _lib.load()
    wire = torch.full((bound + 64,), FILL, dtype=torch.uint8, device="cuda")
    arr = (ctypes.c_void_p * n)(*ptrs)
    used = lib.tk_wire_pack_device_bias(recs, ads, n, arr, ctypes.c_void_p(wire.data_ptr()), bound,
                                        ctypes.c_void_p(_lib.stream_handle(None)))
    torch.cuda.synchronize()
    return int(used), wire.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_packer_equals_host_encoder(device, cases, name):
    import torch
    records, diffs, addends, _ = cases[name]
    bound, host = _host_wire(records, diffs, addends)
    recs, ads, keep = _device_addends(records, diffs, addends)
    dev = [torch.from_numpy(r.copy()).cuda() for r in records]
    ptrs = [t.data_ptr() for t in dev]
    used, w = _pack(recs, ads, len(records), ptrs, bound)
    assert used == len(host), (used, len(host), _lib.load().tk_last_error())
    assert np.array_equal(w[:used], host)
    assert (w[used:] == FILL).all()
    used2, w2 = _pack(recs, ads, len(records), ptrs, bound)
    assert used2 == used and np.array_equal(w2, w)


def _arena(records, shift=0, fill=None):
    """One host buffer for all records: each behind GUARD bytes, `shift` bytes past a 16-byte
    boundary; `fill` None leaves the records' places prefilled like the guards."""
    offs, at = [], 0
    for r in records:
        at = (at + GUARD + 15) // 16 * 16 + shift
        offs.append(at)
        at += r.nbytes
    a = np.full(at + GUARD + 16, FILL, np.uint8)
    if fill is not None:
        for r, o in zip(fill, offs):
            a[o:o + r.nbytes] = r.view(np.uint8)
    return a, offs


def _unpack(records, diffs, addends, wire, arena, offs, mode, skip=()):
    """Gate, upload, decode: (the arena afterwards, [(mismatches, first)] per record)."""
    import torch
    lib = _lib.load()
    n = len(records)
    recs, ads, keep = _device_addends(records, diffs, addends)
    assert lib.tk_wire_check_bias(recs, ads, n, wc.ptr(wire), len(wire)) == 0, lib.tk_last_error()
    dev_wire = torch.from_numpy(wire).cuda()
    dev = torch.from_numpy(arena).cuda()
    assert dev_wire.data_ptr() % 64 == 0 and dev.data_ptr() % 16 == 0
    dst = (ctypes.c_void_p * n)(*[None if i in skip else dev.data_ptr() + o for i, o in enumerate(offs)])
    report = (_lib.tk_wire_mismatch * n)()
    rc = lib.tk_wire_unpack_device_bias(recs, ads, n, ctypes.c_void_p(dev_wire.data_ptr()), len(wire), dst, mode, report,
                                        ctypes.c_void_p(_lib.stream_handle(None)))
    assert rc == 0, lib.tk_last_error()
    return dev.cpu().numpy(), [(int(r.mismatches), int(r.first)) for r in report]


@pytest.mark.parametrize("name", NAMES)
def test_store_equals_the_records(device, cases, name):
    """Destinations 16-byte aligned, 4 bytes past that, and with the first record's destination
    NULL: the bias record is then decoded from a chain that exists in registers only."""
    records, diffs, addends, _ = cases[name]
    _, host = _host_wire(records, diffs, addends)
    for shift in (0, 4):
        arena, offs = _arena(records, shift)
        want, _ = _arena(records, shift, fill=records)
        got, _ = _unpack(records, diffs, addends, host, arena, offs, STORE)
        assert np.array_equal(got, want), (name, shift)      # the records, and every guard byte as it was
    arena, offs = _arena(records)
    want, _ = _arena(records, fill=[np.full_like(records[0], np.int32(-1515870811))] + records[1:])   # 0xA5A5A5A5
    got, _ = _unpack(records, diffs, addends, host, arena, offs, STORE, skip=(0,))
    assert np.array_equal(got, want), name


def _positions(n):
    return sorted({0, min(n - 1, 15), min(n - 1, 16), n // 2, min(n - 1, wc.SEG - 1), min(n - 1, wc.SEG), n - 1})


@pytest.mark.parametrize("name", NAMES)
def test_compare_counts_and_indices(device, cases, name):
    """Equal buffers; one element of the last record changed (that record alone, count 1, that
    index); one element of its predecessor changed (the predecessor alone: the record chained to it
    is compared against the wire's chain, not against the buffer)."""
    records, diffs, addends, _ = cases[name]
    n_rec, n = len(records), len(records[0])
    _, host = _host_wire(records, diffs, addends)
    clean, offs = _arena(records, fill=records)
    got, report = _unpack(records, diffs, addends, host, clean, offs, COMPARE)
    assert report == [NONE] * n_rec
    assert np.array_equal(got, clean)     # compare mode writes nothing
    for k in (n_rec - 1, n_rec - 2):
        for pos in _positions(n):
            arena = clean.copy()
            arena[offs[k] + 4 * pos + 1] ^= 0x10
            _, report = _unpack(records, diffs, addends, host, arena, offs, COMPARE)
            assert report == [(1, pos) if i == k else NONE for i in range(n_rec)], (name, k, pos)


# ---------------------------------------------------------------- through the stack
def _five_channel_block(batch):
    """conv -> bias_add -> requantize -> clip with 5 channels on a 7x7 plane."""
    shape = (batch, 4, 7, 7)
    b = zoo._Builder(29)
    x = zoo._input(b, shape)
    w, bias = b.weight("f.weight", (5, 4, 3, 3)), b.bias("f.bias", 5)
    s_w = b.wscale(5, 36, x.sigma)
    y = qnn.op.conv2d(x.expr, w, relay.const(x.zp, "int32"), relay.const(0, "int32"), relay.const(x.scale, "float32"),
                      relay.const(s_w, "float32"), kernel_size=(3, 3), channels=5, strides=(1, 1), padding=(1, 1))
    y = relay.nn.bias_add(y, bias, axis=1)
    s_out = zoo._requant_out_scale(x.scale, s_w, 36, x.sigma)
    y = qnn.op.requantize(y, relay.const((np.float32(x.scale) * s_w).astype(np.float32), "float32"),
                          relay.const(0, "int32"), relay.const(s_out, "float32"), relay.const(0, "int32"), axis=1,
                          out_dtype="int8")
    y = relay.clip(y, 0.0, 127.0)
    return zoo._finish("five_channel_block", b, zoo.QTensor(y, s_out, 0, 20.0), shape, 29)


GRAPHS = {"lenet5_b2": lambda: (zoo.lenet5(batch=2), 2), "five_channel_block": lambda: (_five_channel_block(3), 3)}


@pytest.mark.parametrize("which", sorted(GRAPHS))
def test_version_3_through_the_stack(device, tmp_path, which):
    from oracle import graph_ref
    model, batch = GRAPHS[which]()
    x = model.sample_inputs(0, batch)
    lib = relay.build(model.mod, target="mi355x", params=model.params)
    gm = graph_executor.GraphModule(lib["default"]())
    try:
        # the precondition of the byte comparison, on the oracle's records: the data rule selects
        # exactly the nn.bias_add records
        exp = graph_ref.calibrate(model.mod, model.params, {model.input_name: x})
        names = [t.name for t in gm.plan.records]
        assert list(exp) == names
        bias_ops = [names.index(o.name) for o in gm.plan.ops if o.op == "nn.bias_add"]
        assert bias_ops and sorted(tf.bias_axes_of_data(exp)[0]) == bias_ops
        assert sorted(graph_executor.PackedCapture.bias_records(gm.plan)) == bias_ops

        gm.set_input(model.input_name, x)
        p1, p2, p3 = (str(tmp_path / f) for f in ("plain.tkt", "packed.tkt", "bias.tkt"))
        gm.dump_trace(p1)
        gm.dump_trace(p2, packed=True)
        gm.dump_trace(p3, packed=True, bias=True)
        plain, v2, v3 = (open(p, "rb").read() for p in (p1, p2, p3))
        assert tf.pack_trace(p1, bias=True) == v3              # host and device writers agree
        assert tf.unpack_trace(p3) == plain
        assert tf.pack_trace(p1) == v2 and len(v3) < len(v2)
        pf = tf.parse_packed(v3)
        assert pf.version == 3 and [i for i, e in enumerate(pf.entries) if e.coding == tf.BIAS] == bias_ops
        assert gm.verify_trace(p3).ok
        rep = gm.replay_trace(p3)
        assert rep.ok and rep.nodes == [] and list(rep.ops) == []
        assert gm.verify_trace(p2).ok                          # version 2 after version 3, one verifier
        gm.load_trace(p3)
        got, want = gm.record_stats(), tf.trace_stats(p3)
        assert list(got) == list(want) and all(got[k].equals(want[k]) for k in want)
        gm.load_trace(p3, shadows=True)
        assert gm.verify_trace(p3, run=False).ok
        # one stored addend value changed: the host gate has nothing to say, the device names the record
        e = pf.entries[bias_ops[0]]
        channel = e.channels - 1
        blob = bytearray(v3)
        blob[pf.addend_off + e.addend_off + 4 * channel] ^= 0x04
        tf.check_trace(np.frombuffer(bytes(blob), np.uint8), [(t.name, t.shape, t.dtype) for t in gm.plan.records])
        rep = gm.verify_trace(bytes(blob))
        assert not rep.ok and rep.first.name == e.name and rep.first.op == "nn.bias_add"
        assert rep.first.count == e.shape[0] * e.plane
        assert rep.first.flat_index == channel * e.plane
    finally:
        gm.close()


def _tracer(packed, bias=False):
    model_fn = zoo.MODELS["lenet5"]
    proto = model_fn(batch=1)

    def build_module(n):
        m = model_fn(batch=n)
        lib = relay.build(m.mod, target="mi355x", params=m.params)
        return graph_executor.GraphModule(lib["default"]())

    return trace_job.GraphModuleTracer(build_module, proto.sample_inputs, model=proto.name,
                                       input_name=proto.input_name, packed=packed, bias=bias)


def test_trace_job_writes_version_3(device, tmp_path, capsys):
    """LeNet-5, 4 samples in 2 chunks: the files are version 3, journal and manifest digests are the
    unpacked job's, and --check --replay accepts them."""
    ref, d = str(tmp_path / "plain"), str(tmp_path / "bias")
    t = _tracer(False)
    try:
        plain = trace_job.run(t, 4, 2, ref)
    finally:
        t.close()
    t = _tracer(True, bias=True)
    try:
        entries = trace_job.run(t, 4, 2, d)
    finally:
        t.close()
    assert [(e.file, e.sample_offset, e.n_samples, e.digest) for e in entries] == \
        [(e.file, e.sample_offset, e.n_samples, e.digest) for e in plain]
    journal = trace_job.Journal(trace_job.journal_file(d, 0)).entries()
    assert all(journal[i]["packed"] is True and journal[i]["version"] == 3 for i in range(2))
    for e in entries:
        assert tf.parse_packed(open(f"{d}/{e.file}", "rb").read()).version == 3
        assert tf.unpack_trace(f"{d}/{e.file}") == open(f"{ref}/{e.file}", "rb").read(), e.file
    with pytest.raises(ValueError):
        _tracer(False, bias=True)
    argv = ["--model", "lenet5", "--samples", "4", "--chunk", "2", "--out-dir", d]
    capsys.readouterr()
    assert trace_job.main(argv + ["--check", "--replay"]) == 0
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert [r["chunk"] for r in lines] == [0, 1] and all(r["ok"] and r["nodes"] == [] for r in lines)
    with pytest.raises(SystemExit):                              # --bias-coding is a mode of --packed
        trace_job.main(argv + ["--bias-coding"])
