"""1-byte records of the trace wire on the device: the encode kernel against the host decoder and
the host encoder's size on the codec cases, and traced runs whose clip records cross the link as
clamps of the record before them against wire off, image byte for byte."""
import ctypes

import numpy as np
import pytest

from tachikoma_amd import _lib, relay, zoo
from tachikoma_amd.contrib import graph_executor
from tachikoma_amd.relay import qnn
from tests import wire_cases as wc
from tests import wire_cases8 as w8

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _collect_after():
    """Modules this file closed (and any cyclic garbage holding device memory) are collected when
    the file is done, not at some later test's expense."""
    yield
    import gc
    gc.collect()


def _device_roundtrip(records, diffs):
    import torch
    lib = _lib.load()
    offs, total = w8.layout(records)
    recs = w8.wire_records(records, diffs, offs)
    src = w8.image_of(records, offs, total)
    bound = lib.tk_wire_bound(recs, len(records))
    assert bound > 0, lib.tk_last_error()
    host_wire = np.zeros(bound, np.uint8)
    host_n = lib.tk_wire_encode_host(recs, len(records), w8.ptr(src), total, w8.ptr(host_wire), bound)
    dev = [torch.from_numpy(r.copy()).cuda() for r in records]
    wire = torch.full((bound,), 0xEE, dtype=torch.uint8, device="cuda")
    ptrs = (ctypes.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
    _lib.check(lib.tk_wire_encode_device(recs, len(records), ptrs, ctypes.c_void_p(wire.data_ptr()), bound,
                                         ctypes.c_void_p(_lib.stream_handle(None))), "tk_wire_encode_device")
    w = wire.cpu().numpy()
    # segments lie in completion order on the device; the size and the widths they state do not differ
    assert host_n == w8.expected_bytes(records, diffs) == w8.parsed_bytes(host_wire, records)
    assert w8.parsed_bytes(w, records) == host_n
    assert w8.stated_widths(w, records) == w8.block_widths(records, diffs)
    out = w8.image_of([np.full_like(r, 0x3C) for r in records], offs, total)
    exact = w[:host_n].copy()   # what the host encoder's size says the decoder may read
    assert lib.tk_wire_decode(recs, len(records), w8.ptr(exact), host_n, w8.ptr(out), total, 0) == 0, lib.tk_last_error()
    assert np.array_equal(out, src)


@pytest.mark.parametrize("n", w8.SIZES)
def test_device_encoder_against_host_decoder(device, n):
    """Every content of the host test, both kinds, at every size (device buffers of odd sizes are
    not all 16-byte aligned: the scalar path too): the device's wire decodes to the source bytes
    within the host encoder's size and states the same widths; an int32 chain and a clamp pair go
    through one launch."""
    for kind in sorted(w8.KINDS):
        rng = np.random.default_rng(n)
        for name, (records, diffs) in sorted(w8.contents(n, kind, rng).items()):
            _device_roundtrip(records, diffs)
        chain, cdiff = wc.contents(n, rng)["diff_chain"]
        pair, pdiff = w8.contents(n, kind, rng)["both_bounds"]
        _device_roundtrip(chain + pair, cdiff + pdiff)


def test_device_encoder_unaligned_sources(device):
    """Record buffers one byte past a 16-byte boundary: every lane takes the byte-wise path."""
    import torch
    lib = _lib.load()
    n = 3 * 256 + 17
    for kind in sorted(w8.KINDS):
        records, diffs = w8.contents(n, kind, np.random.default_rng(8))["off_by_one"]
        offs, total = w8.layout(records)
        recs = w8.wire_records(records, diffs, offs)
        src = w8.image_of(records, offs, total)
        bound = lib.tk_wire_bound(recs, 2)
        dev = [torch.zeros(n + 16, dtype=torch.uint8, device="cuda") for _ in records]
        for t, r in zip(dev, records):
            t[1:1 + n] = torch.from_numpy(r.view(np.uint8).copy()).cuda()
        wire = torch.full((bound,), 0xEE, dtype=torch.uint8, device="cuda")
        ptrs = (ctypes.c_void_p * 2)(*[t.data_ptr() + 1 for t in dev])
        _lib.check(lib.tk_wire_encode_device(recs, 2, ptrs, ctypes.c_void_p(wire.data_ptr()), bound,
                                             ctypes.c_void_p(_lib.stream_handle(None))), "tk_wire_encode_device")
        w = wire.cpu().numpy()
        assert w8.stated_widths(w, records) == w8.block_widths(records, diffs)
        out = w8.image_of([np.zeros_like(r) for r in records], offs, total)
        assert lib.tk_wire_decode(recs, 2, w8.ptr(w), bound, w8.ptr(out), total, 0) == 0, lib.tk_last_error()
        assert np.array_equal(out, src)


BATCH, SHAPE = 3, (3, 8, 9, 9)


def _one_block():
    b = zoo._Builder(11)
    x = zoo._input(b, SHAPE)
    x = zoo.conv_block(b, x, "c", 8, 3, pad=1)      # conv -> bias_add -> requantize -> clip
    return zoo._finish("one_block", b, x, SHAPE, 11)


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


MODELS = {"one_block": _one_block, "residual_pair": _residual_pair, "uint8_block": _uint8_block}


def _images(model, n_inputs, wire, chunks=None):
    lib = relay.build(model.mod, target="mi355x", params=model.params)
    m = graph_executor.GraphModule(lib["default"]())
    m.module.use_graph = True
    m.module.set_trace_wire(wire)
    if chunks:
        _lib.check(m.module.lib.tk_module_set_trace_chunks(m.module.handle, chunks), "tk_module_set_trace_chunks")
    out = []
    for i in range(n_inputs):
        m.set_input(model.input_name, model.sample_inputs(BATCH * i, BATCH))
        m.run(trace=True)
        m.trace_capture().capture_stream.synchronize()   # the only completion call
        out.append(bytes(m.trace_capture().bytes()))
    stats = m.module.wire_stats()
    plan = m.module.plan
    nbytes = lambda t: int(np.prod(t.shape, dtype=np.int64)) * np.dtype(t.dtype).itemsize
    produced = {op.out.name for op in plan.ops}
    int32_bytes = sum(nbytes(t) for t in plan.records if t.dtype == "int32" and t.name in produced)
    clip_bytes = sum(nbytes(op.out) for op in plan.ops if op.op in ("clip", "nn.relu"))
    m.close()
    return out, stats, int32_bytes, clip_bytes


@pytest.mark.parametrize("which", sorted(MODELS))
def test_clip_records_as_clamps_equal_wire_off(device, which, monkeypatch):
    """Batch 3 on 9x9 planes with 8 channels.  Four consecutive traced runs with a different input
    each, completion through the capture stream alone, with the default chunk count, 1 chunk and
    more chunks than records: every whole image equals the wire-off image.  The coded records are
    the int32 records and the clip records; with TK_WIRE_CLAMP=0 at module creation, the int32
    records alone (and the image is the same again)."""
    model = MODELS[which]()
    ref, ref_stats, int32_bytes, clip_bytes = _images(model, 4, False)
    assert len(set(ref)) == 4 and ref_stats == []
    assert int32_bytes > 0 and clip_bytes == BATCH * 8 * 9 * 9
    for chunks in (None, 1, 200):
        got, stats, _, _ = _images(model, 4, True, chunks)
        assert got == ref, chunks
        assert sum(s["coded_raw_bytes"] for s in stats) == int32_bytes + clip_bytes, chunks
        assert all(s["decode_ms"] >= 0 for s in stats)
        if chunks == 1:
            assert len(stats) == 1
    monkeypatch.setenv("TK_WIRE_CLAMP", "0")
    for chunks in (None, 1, 200):
        got, stats, _, _ = _images(model, 4, True, chunks)
        assert got == ref, chunks
        assert sum(s["coded_raw_bytes"] for s in stats) == int32_bytes, chunks
