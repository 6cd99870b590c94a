"""Trace wire on the device: the encode kernel against the host decoder and the host encoder's
size on the codec cases, and traced runs with wire on against wire off, image byte for byte."""
import ctypes

import numpy as np
import pytest

from tachikoma_amd import _lib, relay, zoo
from tachikoma_amd.contrib import graph_executor
from tests import wire_cases as wc

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
    offs, total = wc.layout(records)
    recs = wc.wire_records(records, diffs, offs)
    src = wc.image_of(records, offs, total)
    bound = lib.tk_wire_bound(recs, len(records))
    host_wire = np.zeros(bound, np.uint8)
    host_n = lib.tk_wire_encode_host(recs, len(records), wc.ptr(src), total, wc.ptr(host_wire), bound)
    dev = [torch.from_numpy(r.copy()).cuda() for r in records]
    wire = torch.full((bound,), 0xEE, dtype=torch.uint8, device="cuda")
    ptrs = (ctypes.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
    _lib.check(lib.tk_wire_encode_device(recs, len(records), ptrs, ctypes.c_void_p(wire.data_ptr()), bound,
                                         ctypes.c_void_p(_lib.stream_handle(None))), "tk_wire_encode_device")
    w = wire.cpu().numpy()
    # segments lie in completion order on the device, so the bytes may differ from the host
    # encoder's; the size (every segment by the widths it states) and the decoded image do not
    assert host_n == wc.expected_bytes(records, diffs) == wc.parsed_bytes(host_wire, records)
    assert wc.parsed_bytes(w, records) == host_n
    out = wc.image_of([np.zeros_like(r) for r in records], offs, total)
    exact = w[:host_n].copy()   # what the host encoder's size says the decoder may read
    assert lib.tk_wire_decode(recs, len(records), wc.ptr(exact), host_n, wc.ptr(out), total, 0) == 0, lib.tk_last_error()
    assert np.array_equal(out, src)


@pytest.mark.parametrize("n", wc.SIZES + [2 * wc.SEG + 300])
def test_device_encoder_against_host_decoder(device, n):
    """Every content of the host test at every size (and a record of two full segments and a short
    one): the device's wire decodes to the source bytes within the host encoder's size, and
    its segments, by the widths they state, add up to the same size (equal widths)."""
    for name, (records, diffs) in sorted(wc.contents(n, np.random.default_rng(n)).items()):
        _device_roundtrip(records, diffs)


def _one_block(batch=3):
    b = zoo._Builder(11)
    x = zoo._input(b, (batch, 8, 9, 9))
    x = zoo.conv_block(b, x, "c", 8, 3, pad=1)      # conv -> bias_add -> requantize -> clip
    return zoo._finish("one_block", b, x, (batch, 8, 9, 9), 11)


def _images(model, batch, n_inputs, wire, chunks=None):
    lib = relay.build(model.mod, target="mi355x", params=model.params)
    m = graph_executor.GraphModule(lib["default"]())
    m.module.use_graph = True
    m.module.set_trace_wire(wire)
    if chunks:
        _lib.check(m.module.lib.tk_module_set_trace_chunks(m.module.handle, chunks), "tk_module_set_trace_chunks")
    out = []
    for i in range(n_inputs):
        m.set_input(model.input_name, model.sample_inputs(batch * i, batch))
        m.run(trace=True)
        m.trace_capture().capture_stream.synchronize()   # the only completion call
        out.append(bytes(m.trace_capture().bytes()))
    stats = m.module.wire_stats()
    m.close()
    return out, stats


@pytest.mark.parametrize("which", ["lenet5", "one_block"])
def test_wire_on_equals_wire_off(device, which):
    """Four consecutive traced runs with a different input each (the three slots are reused, the
    two mirrors alternate), completion through the capture stream alone: every whole image equals
    the wire-off image; with 1 chunk and with more chunks than int32 records too."""
    model, batch = (zoo.lenet5(batch=1), 1) if which == "lenet5" else (_one_block(3), 3)
    ref, ref_stats = _images(model, batch, 4, False)
    assert len(set(ref)) == 4 and ref_stats == []
    for chunks in (None, 1, 200):
        got, stats = _images(model, batch, 4, True, chunks)
        assert got == ref, chunks
        coded = sum(s["coded_raw_bytes"] for s in stats)
        assert coded > 0 and all(s["decode_ms"] >= 0 for s in stats)
        if chunks == 1:
            assert len(stats) == 1


def test_wire_runs_back_to_back(device):
    """Runs queued without a synchronisation between them: each waits for the encodes of the one
    before (they read the record buffers it overwrites) and the last image is the last input's;
    a switch to wire off and back in one module keeps giving the same image."""
    model = _one_block(3)
    lib = relay.build(model.mod, target="mi355x", params=model.params)
    m = graph_executor.GraphModule(lib["default"]())
    m.module.use_graph = True
    m.module.set_trace_wire(False)
    m.set_input(model.input_name, model.sample_inputs(6, 3))
    m.run(trace=True)
    m.trace_capture().synchronize()
    ref = bytes(m.trace_capture().bytes())
    for wire in (True, False, True):
        m.module.set_trace_wire(wire)
        for i in range(3):
            m.set_input(model.input_name, model.sample_inputs(3 * i, 3))
            m.run(trace=True)
        m.trace_capture().synchronize()
        assert bytes(m.trace_capture().bytes()) == ref, wire
    m.close()
