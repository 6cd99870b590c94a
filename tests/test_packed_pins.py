"""Pinned bytes of the three trace file versions (no GPU): trace_bytes, pack_trace, pack_trace(bias=True)
and unpack_trace of both packed files, over one small trace built from arithmetic patterns, against the
SHA-256 digests and the packed_info recorded in tests/golden/packed_pins.json.  The trace holds a float32
record, three int32 conv + bias_add pairs -- (2, 3, 7, 7): plane 49, blocks that straddle planes and a
short last block; (1, 5, 3): plane 3, a lane crosses several planes; (1, 2, 16, 32): plane 512, a multiple
of the block -- an int8 and a uint8 record each followed by a clamp of it (the uint8 clamp with one block
the clamp does not reproduce), and an empty record.

``python -m tests.test_packed_pins`` prints the JSON the current tree produces."""
import hashlib
import json
import os

import numpy as np

from tachikoma_amd import trace_format as tf

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_pins.json")


def _i32(shape, mul, mod):
    n = int(np.prod(shape))
    return ((np.arange(n, dtype=np.int64) * mul) % mod - mod // 3).astype(np.int32).reshape(shape)


def _biased(conv, bias):
    """conv + bias on axis 1, int32 wrap-around."""
    b = bias.reshape((1, -1) + (1,) * (conv.ndim - 2))
    return (conv.view(np.uint32) + b.view(np.uint32)).view(np.int32)


def inputs():
    params = {"b0": np.array([1000, -70000, 2 ** 31 - 5], np.int32),
              "b1": (np.arange(5, dtype=np.int32) - 2) * 300007,
              "b2": np.array([-1, 2 ** 24], np.int32),
              "w": (np.arange(24, dtype=np.float32) / 8).reshape(2, 3, 4)}
    records = {"data": (np.arange(2 * 3 * 4 * 4, dtype=np.float32) / 16 - 3).reshape(2, 3, 4, 4)}
    for k, (shape, mul, mod) in enumerate((((2, 3, 7, 7), 7919, 100003), ((1, 5, 3), 65537, 2 ** 31 - 1),
                                           ((1, 2, 16, 32), 31, 251))):
        conv = _i32(shape, mul, mod)
        records[f"%{2 * k}"] = conv
        records[f"%{2 * k + 1}"] = _biased(conv, params[f"b{k}"])
    q = ((np.arange(600, dtype=np.int64) * 37) % 256 - 128).astype(np.int8).reshape(2, 300)
    records["%6"], records["%7"] = q, np.clip(q, -20, 90)
    u = ((np.arange(2 * 3 * 130, dtype=np.int64) * 11) % 256).astype(np.uint8).reshape(2, 3, 130)
    clamped = np.clip(u, 16, 235)
    clamped.reshape(-1)[300] = 3   # block 1 is not a clamp of its predecessor: the raw escape
    records["%8"], records["%9"] = u, clamped
    records["%10"] = np.zeros((0, 4), np.int32)
    meta = {"format": "tachikoma-trace", "version": tf.TRACE_VERSION, "model": "packed_pins", "n_samples": 2}
    return meta, params, records


def _sha(b) -> str:
    return hashlib.sha256(bytes(b)).hexdigest()


def measure():
    v1 = tf.trace_bytes(*inputs())
    v2, v3 = tf.pack_trace(v1), tf.pack_trace(v1, bias=True)
    return {"sha256": {"trace_bytes": _sha(v1), "pack_trace": _sha(v2), "pack_trace_bias": _sha(v3),
                       "unpack_trace": _sha(tf.unpack_trace(v2)), "unpack_trace_bias": _sha(tf.unpack_trace(v3))},
            "packed_info": {"pack_trace": tf.packed_info(v2), "pack_trace_bias": tf.packed_info(v3)}}


def test_packed_pins():
    with open(PINS) as f:
        pins = json.load(f)
    got = measure()
    assert got["sha256"] == pins["sha256"]
    assert got["sha256"]["unpack_trace"] == got["sha256"]["unpack_trace_bias"] == got["sha256"]["trace_bytes"]
    assert got["packed_info"] == pins["packed_info"]
    # the inputs cover what the docstring says they do
    plan = {e["name"]: e for e in got["packed_info"]["pack_trace_bias"]["plan"]}
    assert [plan[f"%{k}"]["coding"] for k in (1, 3, 5)] == [tf.BIAS] * 3
    assert [(plan[k]["coding"], plan[k]["diff"]) for k in ("%7", "%9")] == [(1, 1), (2, 1)]
    assert plan["data"]["coding"] == plan["%10"]["coding"] == "raw"


if __name__ == "__main__":
    print(json.dumps(measure(), indent=1))
