"""Packed trace files on the MI355X: the deterministic device packer (tk_wire_pack_device) byte for
byte against the host encoder, its prefix sum at every tile boundary, and packed dumps / trace jobs
against the unpacked ones through the whole stack (dump_trace(packed=True), GraphModuleTracer(packed=True),
trace_format.pack_trace / unpack_trace)."""
import ctypes

import numpy as np
import pytest

from tachikoma_amd import _lib, relay, shard, trace_job, zoo
from tachikoma_amd import trace_format as tf
from tachikoma_amd.contrib import graph_executor
from tachikoma_amd.relay import qnn
from tachikoma_amd.relay.quantize import quantize
from tests import wire_cases as wc
from tests import wire_cases8 as w8

pytestmark = pytest.mark.gpu

SIZES = sorted(set(wc.SIZES) | set(w8.SIZES))
FILL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _collect_after():
    yield
    import gc
    gc.collect()


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
    return recs, bound, wire[:used].copy()


def _pack(recs, n, ptrs, bound, cap=None):
    """(used, the whole buffer): the buffer is pre-filled, so a byte the packer leaves unwritten
    inside [0, used) differs from the host encoder's zero."""
    import torch
    lib = _lib.load()
    wire = torch.full((bound + 64,), FILL, dtype=torch.uint8, device="cuda")
    arr = (ctypes.c_void_p * n)(*ptrs)
    used = lib.tk_wire_pack_device(recs, n, arr, ctypes.c_void_p(wire.data_ptr()), bound if cap is None else cap,
                                   ctypes.c_void_p(_lib.stream_handle(None)))
    torch.cuda.synchronize()
    return int(used), wire.cpu().numpy()


def _check(records, diffs, dev=None, ptrs=None):
    import torch
    recs, bound, host = _host_wire(records, diffs)
    if ptrs is None:
        dev = [torch.from_numpy(r.copy()).cuda() for r in records]
        ptrs = [t.data_ptr() for t in dev]
    used, w = _pack(recs, len(records), ptrs, bound)
    assert used == len(host), (used, len(host), _lib.load().tk_last_error())
    assert np.array_equal(w[:used], host)
    assert (w[used:] == FILL).all()                      # nothing written past what it reports
    used2, w2 = _pack(recs, len(records), ptrs, bound)   # determinism: the same bytes again
    assert used2 == used and np.array_equal(w2, w)
    return used


@pytest.mark.parametrize("n", SIZES)
def test_packer_equals_host_encoder(device, n):
    """Every content of the codec cases (all width boundaries, INT_MIN and INT_MAX in one block,
    clamps that hold and clamps with escaping blocks, diff and clamp chains) at every size, each
    alone and all three kinds mixed in one call."""
    rng = np.random.default_rng(n)
    mixed, mdiff = [], []
    for name, (records, diffs) in sorted(wc.contents(n, rng).items()):
        _check(records, diffs)
        if name in ("int_min_max", "diff_chain", "diff_wraps"):
            mixed, mdiff = mixed + records, mdiff + diffs
    for kind in sorted(w8.KINDS):
        for name, (records, diffs) in sorted(w8.contents(n, kind, rng).items()):
            _check(records, diffs)
            if name in ("both_bounds", "off_by_one", "block_unclamped", "u8_above_127"):
                mixed, mdiff = mixed + records, mdiff + diffs
    # a clamp chain of three: the clip of a clip
    a, b = w8.contents(n, 1, rng)["both_bounds"][0]
    mixed, mdiff = mixed + [a, b, np.clip(b, -20, 20).astype(np.int8)], mdiff + [0, 1, 1]
    _check(mixed, mdiff)


@pytest.mark.parametrize("shift", [1, 4, 7])
def test_packer_unaligned_sources(device, shift):
    """Sources `shift` bytes past a 16-byte boundary (4: int32 at element alignment only; odd: 1-byte
    records): the byte-wise load path gives the same bytes."""
    import torch
    n = 3 * 256 + 17
    rng = np.random.default_rng(shift)
    records, diffs = [], []
    if shift % 4 == 0:
        r, d = wc.contents(n, rng)["diff_chain"]
        records, diffs = records + r, diffs + d
        r, d = wc.contents(n, rng)["int_min_max"]
        records, diffs = records + r, diffs + d
    for kind in sorted(w8.KINDS):
        r, d = w8.contents(n, kind, rng)["off_by_one"]
        records, diffs = records + r, diffs + d
    dev = [torch.zeros(r.nbytes + 32, dtype=torch.uint8, device="cuda") for r in records]
    for t, r in zip(dev, records):
        assert t.data_ptr() % 16 == 0
        t[shift:shift + r.nbytes] = torch.from_numpy(r.view(np.uint8).copy()).cuda()
    _check(records, diffs, dev, [t.data_ptr() + shift for t in dev])


def test_scan_boundaries(device):
    """One-element records cost one 64-byte segment each, so the segment count is the record
    count: 1, 2, a whole tile, one more (two levels), and one more than two levels cover (three
    levels, which cover every count the format allows).  Every record reads the same four device
    bytes; the host encoder is given the same."""
    import torch
    lib = _lib.load()
    T = lib.tk_wire_pack_tile()
    assert T >= 2
    val = np.array([0x01020304], np.int32)
    dev = torch.from_numpy(val).cuda()
    for n in (1, 2, T, T + 1, 2 * T + 3, T * T + 1):
        recs = (_lib.tk_wire_record * n)()
        raw = np.frombuffer(recs, dtype=np.dtype([("offset", "<i8"), ("n_elems", "<i8"), ("diff", "<i4"), ("kind", "<i4")]))
        raw["offset"], raw["n_elems"], raw["diff"], raw["kind"] = 8, 1, 0, 0
        image = np.zeros(16, np.uint8)
        image[8:12] = val.view(np.uint8)
        bound = lib.tk_wire_bound(recs, n)
        assert bound == (4 * n + 63) // 64 * 64 + 64 * n
        host = np.full(bound, 0x11, np.uint8)
        assert lib.tk_wire_encode_host(recs, n, w8.ptr(image), 16, w8.ptr(host), bound) == bound
        wire = torch.full((bound + 64,), FILL, dtype=torch.uint8, device="cuda")
        ptrs = np.full(n, dev.data_ptr(), np.uint64)
        used = lib.tk_wire_pack_device(recs, n, ptrs.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)),
                                       ctypes.c_void_p(wire.data_ptr()), bound, ctypes.c_void_p(_lib.stream_handle(None)))
        assert used == bound, (n, used, lib.tk_last_error())
        w = wire.cpu().numpy()
        starts = w[:4 * n].view(np.uint32)
        assert np.array_equal(starts, np.arange(n, dtype=np.uint32)), n
        assert np.array_equal(w[:bound], host), n
        assert (w[bound:] == FILL).all()


def test_small_wire_cap_is_refused_before_any_launch(device):
    records, diffs = wc.contents(257, np.random.default_rng(0))["diff_chain"]
    import torch
    recs, bound, host = _host_wire(records, diffs)
    dev = [torch.from_numpy(r.copy()).cuda() for r in records]
    used, w = _pack(recs, len(records), [t.data_ptr() for t in dev], bound, cap=bound - 1)
    assert used == -1 and (w == FILL).all()          # TK_ERR_INVALID_ARG, the buffer untouched
    assert len(host) < bound - 1                     # although the data would have fitted


# ---------------------------------------------------------------- end to end
BATCH, SHAPE = 3, (3, 8, 9, 9)


def _residual_pair():
    b = zoo._Builder(12)
    x = zoo._input(b, SHAPE)
    p = zoo.conv_block(b, x, "p", 8, 3, pad=1, act=None)
    q = zoo.conv_block(b, x, "q", 8, 1, act=None)
    return zoo._finish("residual_pair", b, zoo.qadd(b, p, q, relu=True), SHAPE, 12)   # add -> clip


def _uint8_block():
    """conv -> bias_add -> requantize to uint8 (zero point 100) -> clip(100, 255)."""
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
    return graph_executor.GraphModule(lib["default"]()), model.input_name, model.sample_inputs(0, batch)


def _realized():
    m = zoo.resnet_float(18, batch=1, hw=32)
    lib = relay.build(quantize(m.mod, m.params), target="mi355x")
    return graph_executor.GraphModule(lib["default"]()), "data", m.random_input()


CASES = {
    "lenet5_b1": lambda: _qnn(zoo.lenet5(batch=1), 1),
    "lenet5_b3": lambda: _qnn(zoo.lenet5(batch=3), 3),
    "residual_pair": lambda: _qnn(_residual_pair(), BATCH),
    "uint8_block": lambda: _qnn(_uint8_block(), BATCH),
    "realized_resnet18": _realized,
}


@pytest.mark.parametrize("which", sorted(CASES))
def test_packed_dump_against_unpacked(device, tmp_path, which):
    gm, name, x = CASES[which]()
    try:
        gm.set_input(name, x)
        p1, p2 = str(tmp_path / "plain.tkt"), str(tmp_path / "packed.tkt")
        gm.dump_trace(p1, sample_offset=7)
        gm.dump_trace(p2, packed=True)
        plain, packed = open(p1, "rb").read(), open(p2, "rb").read()
        assert tf.unpack_trace(p2) == plain                    # the reader gives today's file
        assert tf.pack_trace(p1) == packed                     # host and device packers agree
        assert tf.trace_file_digest(p2) == gm.trace_digest() == tf.trace_file_digest(p1)
        codings = {e.coding for e in tf.parse_packed(packed).entries}
        assert 0 in codings and (1 in codings or 2 in codings)
        if which == "realized_resnet18":
            assert tf.RAW in codings and any(e.dtype == "float32" for e in tf.parse_packed(packed).entries)
        if which == "uint8_block":
            assert 2 in codings
        # a second packed dump after another input: the staging and the wire buffer are reused
        gm.set_input(name, np.roll(x, 1, axis=-1))
        gm.dump_trace(p2, packed=True)
        gm.dump_trace(p1)
        assert tf.unpack_trace(p2) == open(p1, "rb").read() != plain
    finally:
        gm.close()


def _tracer(packed):
    model_fn = zoo.MODELS["lenet5"]
    proto = model_fn(batch=1)

    def build_module(n):
        m = model_fn(batch=n)
        lib = relay.build(m.mod, target="mi355x", params=m.params)
        return graph_executor.GraphModule(lib["default"]())

    return trace_job.GraphModuleTracer(build_module, proto.sample_inputs, model=proto.name,
                                       input_name=proto.input_name, packed=packed)


def test_packed_trace_job(device, tmp_path):
    """LeNet-5, 5 samples in chunks of 2 (two chunk sizes, both packers of the first in use): every
    packed chunk unpacks to the file the unpacked job writes, the journal digests are equal, and a
    job stopped after two chunks resumes with the third alone."""
    ref, d = str(tmp_path / "plain"), str(tmp_path / "packed")
    t = _tracer(False)
    try:
        plain = trace_job.run(t, 5, 2, ref)
    finally:
        t.close()
    t = _tracer(True)
    calls = []

    def stopping(offset, n, path):
        if len(calls) == 2:
            raise RuntimeError("stopped")
        calls.append(offset)
        return t(offset, n, path)

    resumed = []

    def counting(offset, n, path):
        resumed.append(offset)
        return t(offset, n, path)

    try:
        with pytest.raises(RuntimeError):
            trace_job.run(stopping, 5, 2, d, packed=True)
        assert sorted(trace_job.Journal(trace_job.journal_file(d, 0)).entries()) == [0, 1]
        entries = trace_job.run(counting, 5, 2, d, packed=True, verify=True)
    finally:
        t.close()
    assert resumed == [4]
    assert [(e.file, e.sample_offset, e.n_samples, e.digest) for e in entries] == \
        [(e.file, e.sample_offset, e.n_samples, e.digest) for e in plain]
    journal = trace_job.Journal(trace_job.journal_file(d, 0)).entries()
    assert all(journal[i]["packed"] is True for i in range(3))
    for e in entries:
        assert tf.unpack_trace(f"{d}/{e.file}") == open(f"{ref}/{e.file}", "rb").read(), e.file
        assert shard.hex64(tf.trace_file_digest(f"{d}/{e.file}")) == e.digest
    assert len(t.stats) == 3 and all(s["bytes"] > 0 and s["write_ms"] >= 0 for s in t.stats)
