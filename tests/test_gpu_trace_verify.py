"""Trace files checked on the MI355X: the device wire decoder (tk_wire_unpack_device) in store and
compare mode against the host encoder's records, the raw compare (tk_compare_device), and the layers
above them: GraphModule.verify_trace / load_trace and trace_job.check / --check."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest

from tachikoma_amd import _lib, relay, trace_job, zoo
from tachikoma_amd import trace_format as tf
from tachikoma_amd.contrib import graph_executor
from tachikoma_amd.relay import qnn
from tachikoma_amd.relay.quantize import quantize
from tests import wire_cases as wc
from tests import wire_cases8 as w8

pytestmark = pytest.mark.gpu

SEG = wc.SEG
BIG = 2 * SEG + 300                       # a chain across three segments with a short last block
SIZES = list(wc.SIZES) + [SEG, SEG + 1, BIG]
FILL, GUARD = 0xA5, 32
NONE = (0, 0xFFFFFFFFFFFFFFFF)
STORE, COMPARE = _lib.TK_WIRE_UNPACK_STORE, _lib.TK_WIRE_UNPACK_COMPARE


def _host_wire(records, diffs):
    lib = _lib.load()
    offs, total = w8.layout(records)
    recs = w8.wire_records(records, diffs, offs)
    src = w8.image_of(records, offs, total)
    bound = lib.tk_wire_bound(recs, len(records))
    assert bound > 0, lib.tk_last_error()
    wire = np.full(bound, 0x11, np.uint8)
    used = lib.tk_wire_encode_host(recs, len(records), w8.ptr(src), total, w8.ptr(wire), bound)
    assert used > 0, lib.tk_last_error()
    return recs, wire[:used].copy()


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


def _unpack(recs, n, wire, arena, offs, mode, skip=()):
    """Gate, upload, decode: (the arena afterwards, [(mismatches, first)] per record)."""
    import torch
    lib = _lib.load()
    assert lib.tk_wire_check(recs, n, w8.ptr(wire), len(wire)) == 0, lib.tk_last_error()
    dev_wire = torch.from_numpy(wire).cuda()
    dev = torch.from_numpy(arena).cuda()
    assert dev_wire.data_ptr() % 64 == 0 and dev.data_ptr() % 16 == 0
    dst = (ctypes.c_void_p * n)(*[None if i in skip else dev.data_ptr() + o for i, o in enumerate(offs)])
    report = (_lib.tk_wire_mismatch * n)()
    rc = lib.tk_wire_unpack_device(recs, n, ctypes.c_void_p(dev_wire.data_ptr()), len(wire), dst, mode, report,
                                   ctypes.c_void_p(_lib.stream_handle(None)))
    assert rc == 0, lib.tk_last_error()
    return dev.cpu().numpy(), [(int(r.mismatches), int(r.first)) for r in report]


def _store_roundtrip(records, diffs, shift=0, wire=None):
    recs, host = _host_wire(records, diffs)
    arena, offs = _arena(records, shift)
    want, _ = _arena(records, shift, fill=records)
    got, _ = _unpack(recs, len(records), host if wire is None else wire, arena, offs, STORE)
    assert np.array_equal(got, want)      # the records, and every guard byte as it was


def _mixed(n, rng):
    mixed, mdiff = [], []
    for name in ("int_min_max", "diff_chain", "diff_wraps"):
        r, d = wc.contents(n, rng)[name]
        mixed, mdiff = mixed + r, mdiff + d
    for kind in sorted(w8.KINDS):
        for name in ("both_bounds", "off_by_one", "block_unclamped"):
            r, d = w8.contents(n, kind, rng)[name]
            mixed, mdiff = mixed + r, mdiff + d
    a, b = w8.contents(n, 1, rng)["both_bounds"][0]
    return mixed + [a, b, np.clip(b, -20, 20).astype(np.int8)], mdiff + [0, 1, 1]   # the clip of a clip


def test_decoder_narrowest(device):
    """One int32 record of one full block and one short one: the first thing to run on a new build."""
    rng = np.random.default_rng(0)
    _store_roundtrip(*wc.contents(257, rng)["range_65535"])


@pytest.mark.parametrize("n", SIZES)
def test_store_equals_the_records(device, n):
    rng = np.random.default_rng(n)
    for name, (records, diffs) in sorted(wc.contents(n, rng).items()):
        _store_roundtrip(records, diffs)
    for kind in sorted(w8.KINDS):
        for name, (records, diffs) in sorted(w8.contents(n, kind, rng).items()):
            _store_roundtrip(records, diffs)
    _store_roundtrip(*_mixed(n, rng))


def test_table_order_is_followed(device):
    """The wire of the live device encoder, whose segments lie in completion order."""
    import torch
    lib = _lib.load()
    records, diffs = _mixed(BIG, np.random.default_rng(3))
    offs, total = w8.layout(records)
    recs = w8.wire_records(records, diffs, offs)
    bound = lib.tk_wire_bound(recs, len(records))
    dev = [torch.from_numpy(r.copy()).cuda() for r in records]
    wire = torch.zeros(bound, dtype=torch.uint8, device="cuda")
    ptrs = (ctypes.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
    _lib.check(lib.tk_wire_encode_device(recs, len(records), ptrs, ctypes.c_void_p(wire.data_ptr()), bound,
                                         ctypes.c_void_p(_lib.stream_handle(None))), "tk_wire_encode_device")
    w = wire.cpu().numpy()
    _store_roundtrip(records, diffs, wire=w[:w8.parsed_bytes(w, records)].copy())


@pytest.mark.parametrize("shift", [1, 4, 7])
def test_unaligned_destinations(device, shift):
    n = 3 * 256 + 17
    rng = np.random.default_rng(shift)
    records, diffs = [], []
    if shift % 4 == 0:
        for name in ("diff_chain", "int_min_max"):
            r, d = wc.contents(n, rng)[name]
            records, diffs = records + r, diffs + d
    for kind in sorted(w8.KINDS):
        r, d = w8.contents(n, kind, rng)["off_by_one"]
        records, diffs = records + r, diffs + d
    _store_roundtrip(records, diffs, shift=shift)
    recs, host = _host_wire(records, diffs)
    arena, offs = _arena(records, shift, fill=records)
    arena[offs[-1] + n - 1] ^= 0x40
    _, report = _unpack(recs, len(records), host, arena, offs, COMPARE)
    assert report == [NONE] * (len(records) - 1) + [(1, n - 1)]


@pytest.mark.parametrize("n", [257, BIG])
def test_compare_equal(device, n):
    records, diffs = _mixed(n, np.random.default_rng(n))
    recs, host = _host_wire(records, diffs)
    arena, offs = _arena(records, fill=records)
    got, report = _unpack(recs, len(records), host, arena, offs, COMPARE)
    assert report == [NONE] * len(records)
    assert np.array_equal(got, arena)     # compare mode writes nothing


def _chain(kind):
    rng = np.random.default_rng(17)
    if kind == "int32":
        return wc.contents(BIG, rng)["diff_chain"]
    a, b = w8.contents(BIG, 1, rng)["both_bounds"][0]
    return [a, b, np.clip(b, -20, 20).astype(np.int8)], [0, 1, 1]


@pytest.mark.parametrize("kind", ["int32", "int8"])
def test_compare_one_element_wrong_does_not_cascade(device, kind):
    records, diffs = _chain(kind)
    es = records[0].itemsize
    recs, host = _host_wire(records, diffs)
    clean, offs = _arena(records, fill=records)
    for k in range(3):
        for pos in (0, 255, 256, SEG - 1, SEG, BIG - 1):
            arena = clean.copy()
            arena[offs[k] + pos * es] ^= 0x10
            _, report = _unpack(recs, 3, host, arena, offs, COMPARE)
            assert report == [(1, pos) if i == k else NONE for i in range(3)], (k, pos, report)
    for k, (p0, p1) in ((0, (300, SEG + 5)), (1, (SEG - 1, 2 * SEG + 299)), (2, (2 * SEG, 17))):
        arena = clean.copy()
        arena[offs[k] + p0 * es] ^= 0x01
        arena[offs[k] + p1 * es + es - 1] ^= 0x80
        _, report = _unpack(recs, 3, host, arena, offs, COMPARE)
        assert report == [(2, min(p0, p1)) if i == k else NONE for i in range(3)], (k, report)


@pytest.mark.parametrize("kind", ["int32", "int8"])
def test_skipped_middle_record(device, kind):
    records, diffs = _chain(kind)
    es = records[0].itemsize
    recs, host = _host_wire(records, diffs)
    arena, offs = _arena(records)
    got, _ = _unpack(recs, 3, host, arena, offs, STORE, skip={1})
    untouched = np.full(records[1].nbytes, FILL, np.uint8).view(records[1].dtype)
    want, _ = _arena(records, fill=[records[0], untouched, records[2]])
    assert np.array_equal(got, want)      # the outer two stored, the skipped one and the guards untouched
    bad = want.copy()
    bad[offs[2] + (SEG + 1) * es] ^= 0x04
    got, report = _unpack(recs, 3, host, bad, offs, COMPARE, skip={1})
    assert report == [NONE, NONE, (1, SEG + 1)] and np.array_equal(got, bad)


def test_unpack_argument_checks(device):
    import torch
    lib = _lib.load()
    records, diffs = wc.contents(257, np.random.default_rng(0))["diff_chain"]
    recs, host = _host_wire(records, diffs)
    wire = torch.from_numpy(np.concatenate([host, np.zeros(64, np.uint8)])).cuda()
    bufs = [torch.full((r.nbytes + 16,), FILL, dtype=torch.uint8, device="cuda") for r in records]
    dst = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in bufs])
    report = (_lib.tk_wire_mismatch * 3)()
    s = ctypes.c_void_p(_lib.stream_handle(None))

    def call(recs=recs, n=3, wire_ptr=wire.data_ptr(), nbytes=len(host), dst=dst, mode=STORE, report=report):
        return lib.tk_wire_unpack_device(recs, n, ctypes.c_void_p(wire_ptr), nbytes, dst, mode, report, s)

    assert call(wire_ptr=wire.data_ptr() + 16) == -1           # not 64-byte aligned
    assert call(nbytes=63) == -1                               # below the table
    assert call(n=0) == -1 and call(mode=2) == -1 and call(mode=COMPARE, report=None) == -1
    odd = (ctypes.c_void_p * 3)(bufs[0].data_ptr() + 2, bufs[1].data_ptr(), bufs[2].data_ptr())
    assert call(dst=odd) == -1                                 # an int32 record at a 2-byte boundary
    bad = w8.wire_records(records, diffs, [0, 0, 0])
    bad[1].n_elems += 1
    assert call(recs=bad) == -1                                # diff after a record of another size
    bad = w8.wire_records(records, diffs, [0, 0, 0])
    bad[2].kind = 1
    assert call(recs=bad) == -1                                # ... of another kind
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == FILL).all() for t in bufs)  # nothing was launched
    assert call() == 0


# ---------------------------------------------------------------- tk_compare_device
@pytest.mark.parametrize("dtype", [np.float32, np.int16, np.int64])
def test_compare_device(device, dtype):
    import torch
    lib = _lib.load()
    es = np.dtype(dtype).itemsize
    s = ctypes.c_void_p(_lib.stream_handle(None))
    rng = np.random.default_rng(es)

    def compare(a, b, sa, sb):
        """a and b placed sa / sb bytes past a 16-byte boundary."""
        ta = torch.zeros(a.nbytes + 48, dtype=torch.uint8, device="cuda")
        tb = torch.zeros(b.nbytes + 48, dtype=torch.uint8, device="cuda")
        ta[sa:sa + a.nbytes] = torch.from_numpy(a.view(np.uint8).copy()).cuda()
        tb[sb:sb + b.nbytes] = torch.from_numpy(b.view(np.uint8).copy()).cuda()
        rep = _lib.tk_wire_mismatch()
        assert lib.tk_compare_device(ctypes.c_void_p(ta.data_ptr() + sa), ctypes.c_void_p(tb.data_ptr() + sb), len(a), es,
                                     ctypes.byref(rep), s) == 0, lib.tk_last_error()
        return int(rep.mismatches), int(rep.first)

    for n in (1, 3, 4097):
        a = (rng.standard_normal(n) * 1000).astype(dtype)
        for sa, sb in ((0, 0), (es, es), (es, 0), (4, 8), (1, 3)):
            assert compare(a, a.copy(), sa, sb) == NONE, (n, sa, sb)
            one = a.copy()
            one.view(np.uint8)[(n - 1) * es + es - 1] ^= 0x80      # the sign bit of the last element
            assert compare(a, one, sa, sb) == (1, n - 1), (n, sa, sb)
            if n >= 3:
                two = one.copy()
                two.view(np.uint8)[(n // 2) * es] ^= 0x01
                assert compare(a, two, sa, sb) == (2, n // 2), (n, sa, sb)


def test_compare_device_batch(device):
    import torch
    lib = _lib.load()
    rng = np.random.default_rng(1)
    arrays = [rng.standard_normal(5000).astype(np.float32), rng.integers(-9, 9, 3, dtype=np.int64),
              np.zeros(0, np.int16), rng.integers(-100, 100, 4097, dtype=np.int64).astype(np.int16),
              rng.integers(0, 255, 33, dtype=np.int64).astype(np.uint8)]
    other = [a.copy() for a in arrays]
    other[0][4999] += 1
    other[0][1234] += 1
    other[3][4096] += 1
    ta = [torch.from_numpy(a).cuda() for a in arrays]
    tb = [torch.from_numpy(a).cuda() for a in other]
    n = len(arrays)
    exp = (ctypes.c_void_p * n)(*[t.data_ptr() if t.numel() else None for t in ta])
    got = (ctypes.c_void_p * n)(*[t.data_ptr() if t.numel() else None for t in tb])
    cnt = (ctypes.c_int64 * n)(*[len(a) for a in arrays])
    es = (ctypes.c_int32 * n)(*[a.itemsize for a in arrays])
    rep = (_lib.tk_wire_mismatch * n)()
    s = ctypes.c_void_p(_lib.stream_handle(None))
    assert lib.tk_compare_device_batch(exp, got, cnt, es, n, rep, s) == 0, lib.tk_last_error()
    assert [(int(r.mismatches), int(r.first)) for r in rep] == [(2, 1234), NONE, NONE, (1, 4096), NONE]
    es[1] = 3
    assert lib.tk_compare_device_batch(exp, got, cnt, es, n, rep, s) == -1


# ---------------------------------------------------------------- end to end
BATCH, SHAPE = 3, (3, 8, 9, 9)


def _residual_pair():
    b = zoo._Builder(12)
    x = zoo._input(b, SHAPE)
    p = zoo.conv_block(b, x, "p", 8, 3, pad=1, act=None)
    q = zoo.conv_block(b, x, "q", 8, 1, act=None)
    return zoo._finish("residual_pair", b, zoo.qadd(b, p, q, relu=True), SHAPE, 12)


def _uint8_block():
    b = zoo._Builder(13)
    x = zoo._input(b, SHAPE)
    w, bias = b.weight("u.weight", (8, 8, 3, 3)), b.bias("u.bias", 8)
    s_w = b.wscale(8, 72, x.sigma)
    y = qnn.op.conv2d(x.expr, w, relay.const(x.zp, "int32"), relay.const(0, "int32"), relay.const(x.scale, "float32"),
                      relay.const(s_w, "float32"), kernel_size=(3, 3), channels=8, strides=(1, 1), padding=(1, 1))
    y = relay.nn.bias_add(y, bias, axis=1)
    s_out = zoo._requant_out_scale(x.scale, s_w, 72, x.sigma)
    y = qnn.op.requantize(y, relay.const((np.float32(x.scale) * s_w).astype(np.float32), "float32"),
                          relay.const(0, "int32"), relay.const(s_out, "float32"), relay.const(100, "int32"), axis=1,
                          out_dtype="uint8")
    y = relay.clip(y, 100.0, 255.0)
    return zoo._finish("uint8_block", b, zoo.QTensor(y, s_out, 100, 20.0), SHAPE, 13)


def _qnn(model, batch):
    lib = relay.build(model.mod, target="mi355x", params=model.params)
    return (graph_executor.GraphModule(lib["default"]()), model.input_name, model.sample_inputs(0, batch),
            model.sample_inputs(batch, batch))


def _realized():
    m = zoo.resnet_float(18, batch=1, hw=32)
    lib = relay.build(quantize(m.mod, m.params), target="mi355x")
    x = m.random_input()
    return graph_executor.GraphModule(lib["default"]()), "data", x, np.ascontiguousarray(x[..., ::-1]) * np.float32(0.5)


CASES = {
    "lenet5_b1": lambda: _qnn(zoo.lenet5(batch=1), 1),
    "lenet5_b3": lambda: _qnn(zoo.lenet5(batch=3), 3),
    "residual_pair": lambda: _qnn(_residual_pair(), BATCH),
    "uint8_block": lambda: _qnn(_uint8_block(), BATCH),
    "realized_resnet18": _realized,
}


@pytest.fixture(scope="module")
def graphs():
    """Built once per file, closed when the file is done."""
    built = {}

    def get(which):
        if which not in built:
            built[which] = CASES[which]()
        return built[which]

    yield get
    for gm, *_ in built.values():
        gm.close()
    import gc
    gc.collect()


def _dump_pair(gm, name, x, d, tag):
    gm.set_input(name, x)
    p1, p2 = os.path.join(d, f"{tag}.plain.tkt"), os.path.join(d, f"{tag}.packed.tkt")
    gm.dump_trace(p1)
    gm.dump_trace(p2, packed=True)
    return p1, p2


def _modified(plain_path, records, pos, flat, d, tag):
    """The version-1 file with element `flat` of record `pos` changed on the host, and the packed
    file pack_trace derives from it: (paths, the value now in the files)."""
    blob = bytearray(open(plain_path, "rb").read())
    ct = tf.check_trace(bytes(blob), records)
    e = ct.entries[pos]
    dt = np.dtype(e.dtype)
    at = ct.records_off + e.raw_off + flat * dt.itemsize
    old = np.frombuffer(bytes(blob[at:at + dt.itemsize]), dt)[0]
    if dt.kind == "f":
        new = dt.type(old + 1.5)
    else:
        new = dt.type(old - 1 if old == np.iinfo(dt).max else old + 1)
    assert new != old
    blob[at:at + dt.itemsize] = np.array([new], dt).tobytes()
    p1, p2 = os.path.join(d, f"{tag}.plain.tkt"), os.path.join(d, f"{tag}.packed.tkt")
    open(p1, "wb").write(bytes(blob))
    open(p2, "wb").write(tf.pack_trace(bytes(blob)))
    return (p1, p2), new, old


@pytest.mark.parametrize("which", sorted(CASES))
def test_verify_trace_end_to_end(device, tmp_path, graphs, which):
    gm, name, xa, xb = graphs(which)
    d = str(tmp_path)
    records = [(t.name, t.shape, t.dtype) for t in gm.plan.records]
    inputs = {t.name for t in gm.plan.inputs}
    a = _dump_pair(gm, name, xa, d, "a")
    for path in a:
        rep = gm.verify_trace(path)
        assert rep.ok and rep.first is None and rep.mismatches == [] and rep.params_equal, (path, rep)
        assert rep.n_records == len(gm.plan.records) and rep.params_differing == []
        assert rep.stats["file_bytes"] == os.path.getsize(path) and rep.stats["upload_bytes"] > 0
    assert gm.verify_trace(a[1]).stats["packed"] is True and gm.verify_trace(a[0]).stats["packed"] is False
    assert gm.verify_trace(open(a[1], "rb").read()).ok          # bytes as well as a path
    # another input through the same module, the files verified in both orders: the run must start
    # from the file's input, shadow and all, not from what the module last saw
    b = _dump_pair(gm, name, xb, d, "b")
    assert open(a[0], "rb").read() != open(b[0], "rb").read()
    for path in (a[1], b[0], a[0], b[1], a[1]):
        assert gm.verify_trace(path).ok, path
    # as the buffers stand (they hold a's records now), b's file differs and a's does not
    assert gm.verify_trace(a[0], run=False).ok and not gm.verify_trace(b[1], run=False).ok
    # one element changed in the file
    entries = tf.parse_packed(open(a[1], "rb").read()).entries
    conv = next(i for i, e in enumerate(entries[:-1]) if e.coding == 0 and not e.diff and
                entries[i + 1].coding == 0 and entries[i + 1].diff)
    clip = next((i for i, e in enumerate(entries) if e.coding in (1, 2) and e.diff and e.name not in inputs), None)
    assert clip is not None or which == "realized_resnet18"      # the qnn graphs all end a block in a clip
    targets = [conv] + ([clip] if clip is not None else [])
    if which == "realized_resnet18":
        targets.append(max(i for i, e in enumerate(entries) if e.dtype == "float32" and e.name not in inputs))
    for pos in targets:
        e = entries[pos]
        flat = tf._n_elems(e.shape) * 2 // 3
        paths, new, old = _modified(a[0], records, pos, flat, d, f"m{pos}")
        for path in paths:
            rep = gm.verify_trace(path)
            assert not rep.ok and rep.params_equal and len(rep.mismatches) == 1, (path, rep)
            m = rep.mismatches[0]
            assert rep.first is m
            assert (m.name, m.position, m.dtype, m.shape, m.count, m.flat_index) == \
                (e.name, pos, e.dtype, e.shape, 1, flat), m
            assert m.first_index == tuple(int(i) for i in np.unravel_index(flat, e.shape))
            assert m.op == next(o.op for o in gm.plan.ops if o.name == e.name)
            expected, got = rep.detail(m)
            assert expected == new and got == old, (expected, got, new, old)


def test_verify_trace_params_differ(device, tmp_path, graphs):
    gm, name, xa, _ = graphs("lenet5_b3")
    a = _dump_pair(gm, name, xa, str(tmp_path), "a")
    conv = next(o for o in gm.plan.ops if o.op == "qnn.conv2d")
    wname = conv.inputs[1]
    w = gm.module.buffers[wname].cpu().numpy()
    changed = w.copy()
    changed.reshape(-1)[0] += 1 if changed.reshape(-1)[0] < 127 else -1
    gm.set_input(wname, changed)
    try:
        for path in a:
            rep = gm.verify_trace(path)
            assert not rep.ok and not rep.params_equal and rep.params_differing == [wname]
            assert rep.first is not None and rep.first.name == conv.name and rep.first.op == "qnn.conv2d"
    finally:
        gm.set_input(wname, w)
    assert all(gm.verify_trace(path).ok for path in a)


def test_verify_trace_refusals(device, tmp_path, graphs):
    d = str(tmp_path)
    gm, name, xa, _ = graphs("residual_pair")
    a = _dump_pair(gm, name, xa, d, "a")
    other, oname, ox, _ = graphs("uint8_block")
    b1, n1, x1, _ = graphs("lenet5_b1")
    b3, n3, x3, _ = graphs("lenet5_b3")
    for path in a:
        with pytest.raises(ValueError, match="another graph"):
            other.verify_trace(path)
    for path in _dump_pair(b1, n1, x1, d, "b1"):
        with pytest.raises(ValueError, match="another graph"):     # another batch size
            b3.verify_trace(path)
        with pytest.raises(ValueError, match="another graph"):
            b3.load_trace(path)
    packed = open(a[1], "rb").read()
    assert gm.verify_trace(packed).ok
    uploads = gm.trace_verifier().uploads
    assert uploads > 0
    with pytest.raises(ValueError):
        gm.verify_trace(packed[:-100])
    pf = tf.parse_packed(packed)
    bad = bytearray(packed)
    bad[pf.wire_off + 4:pf.wire_off + 8] = b"\xff\xff\xff\xff"
    with pytest.raises(ValueError, match="tk_wire_check"):
        gm.verify_trace(bytes(bad))
    with pytest.raises(ValueError):
        gm.verify_trace(b"TKTRACE\0" + bytes(48))               # a header and nothing else
    assert gm.trace_verifier().uploads == uploads                 # the device saw none of them
    assert gm.verify_trace(packed).ok


@pytest.mark.parametrize("which", ["lenet5_b3", "realized_resnet18"])
def test_load_trace(device, tmp_path, graphs, which):
    gm, name, xa, xb = graphs(which)
    a = _dump_pair(gm, name, xa, str(tmp_path), "a")
    for path in a:
        gm.set_input(name, xb)
        gm.run()
        want = tf.read_trace(path).records
        assert any(not np.array_equal(gm.get_node_output(k).numpy(), v) for k, v in want.items())
        gm.load_trace(path)
        for k, v in want.items():
            assert np.array_equal(gm.get_node_output(k).numpy(), v), (path, k)


# ---------------------------------------------------------------- trace job
def _tracer(packed):
    model_fn = zoo.MODELS["lenet5"]
    proto = model_fn(batch=1)

    def build_module(n):
        m = model_fn(batch=n)
        lib = relay.build(m.mod, target="mi355x", params=m.params)
        return graph_executor.GraphModule(lib["default"]())

    return trace_job.GraphModuleTracer(build_module, proto.sample_inputs, model=proto.name,
                                       input_name=proto.input_name, packed=packed)


@pytest.mark.parametrize("packed", [False, True])
def test_trace_job_check(device, tmp_path, packed, capsys):
    d = str(tmp_path / "job")
    t = _tracer(packed)
    try:
        trace_job.run(t, 5, 2, d)
        rows = trace_job.check(t, d)
        assert [r["chunk"] for r in rows] == [0, 1, 2] and all(r["ok"] for r in rows), rows
        assert all(r["n_mismatched"] == 0 and r["first"] is None and r["params_equal"] and
                   r["packed"] is packed and r["file_bytes"] > 0 for r in rows)
        assert trace_job.main(["--model", "lenet5", "--samples", "5", "--chunk", "2", "--out-dir", d, "--check"]) == 0
        lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
        assert [r["chunk"] for r in lines] == [0, 1, 2] and all(r["ok"] for r in lines)
        # chunk 1's file replaced by one with a changed record
        path = trace_job.chunk_file(d, 0, 1)
        plain = bytes(tf.unpack_trace(path)) if packed else open(path, "rb").read()
        trace = tf.read_trace(plain)
        names = list(trace.records)
        pos = next(i for i, k in enumerate(names) if trace.records[k].dtype == np.int32)
        records = [(k, v.shape, str(v.dtype)) for k, v in trace.records.items()]
        (p1, p2), _, _ = _modified_bytes(plain, records, pos, 5, str(tmp_path))
        shutil.copyfile(p2 if packed else p1, path)
        rows = trace_job.check(t, d)
        assert [r["ok"] for r in rows] == [True, False, True], rows
        assert rows[1]["n_mismatched"] == 1 and rows[1]["first"]["name"] == names[pos]
        assert rows[1]["first"]["first_index"] == [int(i) for i in np.unravel_index(5, trace.records[names[pos]].shape)]
        os.remove(trace_job.chunk_file(d, 0, 2))
        rows = trace_job.check(t, d)
        assert [r["ok"] for r in rows] == [True, False, False] and "error" in rows[2]
    finally:
        t.close()
    assert trace_job.main(["--model", "lenet5", "--samples", "5", "--chunk", "2", "--out-dir", d, "--check"]) == 1


def _modified_bytes(plain, records, pos, flat, d):
    src = os.path.join(d, "src.tkt")
    open(src, "wb").write(plain)
    return _modified(src, records, pos, flat, d, "mod")
