"""Bias coding of the trace wire on the device: the encode kernel with a device addend against the
host decoder with a host addend and the host encoder's size, and traced runs of modules whose
bias_add records are coded with the plan's bias snapshot against wire off, image byte for byte,
also after the params change under the plan."""
import ctypes

import numpy as np
import pytest

from tachikoma_amd import _lib, relay, zoo
from tachikoma_amd.contrib import graph_executor
from tests import wire_cases as wc
from tests import wire_cases_bias as wb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _collect_after():
    yield
    import gc
    gc.collect()


def _device_roundtrip(records, diffs, addends, flat, shift=0):
    """Encodes on the device from buffers `shift` bytes past a 16-byte boundary (4: every lane takes
    the element path), decodes on the host; returns the wire bytes."""
    import torch
    lib = _lib.load()
    offs, total = wc.layout(records)
    host_recs, host_ads = wb.wire_records(records, diffs, addends, offs)
    src = wc.image_of(records, offs, total)
    bound = lib.tk_wire_bound(host_recs, len(records))
    assert bound > 0, lib.tk_last_error()
    host_wire = np.zeros(bound, np.uint8)
    host_n = lib.tk_wire_encode_host_bias(host_recs, host_ads, len(records), wc.ptr(src), total, wc.ptr(host_wire), bound)
    assert host_n == wb.expected_bytes(records, diffs, addends)
    dev = []
    for r in records:
        t = torch.zeros(4 * len(r) + 32, dtype=torch.uint8, device="cuda")
        t[shift:shift + 4 * len(r)] = torch.from_numpy(r.view(np.uint8).copy()).cuda()
        dev.append(t)
    dev_addends = {i: torch.from_numpy(ad[2].copy()).cuda() for i, ad in enumerate(addends) if ad is not None}
    dev_recs, dev_ads = wb.wire_records(records, diffs, addends, offs, {i: t.data_ptr() for i, t in dev_addends.items()})
    wire = torch.full((bound,), 0xEE, dtype=torch.uint8, device="cuda")
    ptrs = (ctypes.c_void_p * len(dev))(*[t.data_ptr() + shift for t in dev])
    _lib.check(lib.tk_wire_encode_device_bias(dev_recs, dev_ads, len(records), ptrs, ctypes.c_void_p(wire.data_ptr()),
                                              bound, ctypes.c_void_p(_lib.stream_handle(None))), "tk_wire_encode_device_bias")
    w = wire.cpu().numpy()
    # segments lie in completion order on the device; the size by the widths they state is the host's
    assert wc.parsed_bytes(w, records) == host_n
    out = wc.image_of([np.zeros_like(r) for r in records], offs, total)
    exact = w[:host_n].copy()
    assert lib.tk_wire_decode_bias(host_recs, host_ads, len(records), wc.ptr(exact), host_n, wc.ptr(out), total,
                                   0) == 0, lib.tk_last_error()
    assert np.array_equal(out, src)
    return host_n


@pytest.mark.parametrize("shift", [0, 4], ids=["aligned", "element_path"])
def test_device_encoder_with_addend(device, shift):
    """The grid and the other cases of the host test: the device's wire decodes to the source bytes
    on the host within the host encoder's size, and its segments add up to that size."""
    for name, (records, diffs, addends, flat) in sorted(wb.cases(np.random.default_rng(7)).items()):
        _device_roundtrip(records, diffs, addends, flat, shift)


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
    return zoo._finish("residual_pair", b, zoo.qadd(b, p, q, relu=True), SHAPE, 12)


MODELS = {"one_block": (_one_block, BATCH), "residual_pair": (_residual_pair, BATCH),
          "lenet5": (lambda: zoo.lenet5(batch=1), 1)}   # dense blocks: plane 1


def _images(model, batch, n_inputs, wire, chunks=None, new_params=None):
    """The images of n_inputs traced runs and the last run's summed wire bytes; with `new_params`,
    also the image of one more run (the last input again) after load_params."""
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
    wire_bytes = sum(s["wire_bytes"] for s in m.module.wire_stats())
    after = None
    if new_params is not None:
        m.load_params(relay.save_param_dict(new_params))
        m.run(trace=True)
        m.trace_capture().capture_stream.synchronize()
        after = bytes(m.trace_capture().bytes())
    m.close()
    return out, wire_bytes, after


def _other_biases(params):
    """The same params with every int32 vector (the biases) changed: reversed, and one value moved."""
    out = {k: np.asarray(v) for k, v in params.items()}
    changed = 0
    for k, v in out.items():
        if v.dtype == np.int32 and v.ndim == 1:
            w = np.ascontiguousarray(v[::-1]).copy()
            w[0] += 12345
            out[k] = w
            changed += 1
    assert changed
    return out


@pytest.mark.parametrize("which", sorted(MODELS))
def test_bias_coded_runs_equal_wire_off(device, which, monkeypatch):
    """Four consecutive traced runs with a different input each, completion through the capture
    stream alone, at the default chunk count, 1 chunk and 200 chunks (a conv and its bias_add then
    lie in different chunks): every whole image equals the wire-off image, the wire carries fewer
    bytes than that of the same module created under TK_WIRE_BIAS=0 (whose images are equal too),
    and after load_params changes the biases under the plan's snapshot the image still equals wire
    off for the new params."""
    make, batch = MODELS[which]
    model = make()
    p2 = _other_biases(model.params)
    ref, ref_wire, ref_after = _images(model, batch, 4, False, None, p2)
    assert len(set(ref)) == 4 and ref_wire == 0 and ref_after != ref[3]
    for chunks in (None, 1, 200):
        got, wire_bytes, after = _images(model, batch, 4, True, chunks, p2)
        assert got == ref, chunks
        assert after == ref_after, chunks
        with monkeypatch.context() as mp:
            mp.setenv("TK_WIRE_BIAS", "0")
            plain, plain_bytes, plain_after = _images(model, batch, 4, True, chunks, p2)
        assert plain == ref and plain_after == ref_after, chunks
        assert 0 < wire_bytes < plain_bytes, (chunks, wire_bytes, plain_bytes)
