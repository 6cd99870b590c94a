"""Per-record statistics on the host (tachikoma_amd/trace_format.py: RecordStats, record_stats,
trace_stats, the ``stats`` command; tachikoma_amd/trace_job.py: merge_stats).  Everything is an
integer, so every check is equality with plain numpy written from the definitions: count, sum
modulo 2^64, min, max, bits[b] = elements whose magnitude has bit length b (b(0) = 0, b(x) =
floor(log2|x|) + 1, 32 for INT32_MIN), values[v - dtype_min] for the 1-byte dtypes.  The device
kernel is covered by tests/test_gpu_record_stats.py and tests/test_gpu_module_stats.py."""
import concurrent.futures
import json

import numpy as np
import pytest

from tachikoma_amd import trace_job, zoo
from tachikoma_amd import trace_format as tf
from tests import stats_cases as sc

I32_MIN, I32_MAX = sc.I32_MIN, sc.I32_MAX
assert_is = sc.assert_is


def arrays():
    rng = np.random.default_rng(7)
    return {
        "i32_extremes": np.array([I32_MIN, I32_MAX, 0, -1, 1, 2, 3, 4, -4, 2 ** 30, -2 ** 30, 2 ** 31 - 2], np.int32),
        "i32_random": rng.integers(I32_MIN, I32_MAX, 5000, dtype=np.int64, endpoint=True).astype(np.int32),
        "i32_small": rng.integers(-3, 4, (7, 11)).astype(np.int32),
        "i8_extremes": np.array([-128, 127, 0, -1, 1, 64, -64, 63], np.int8),
        "i8_random": rng.integers(-128, 128, 3000).astype(np.int8),
        "u8_extremes": np.array([0, 255, 1, 127, 128, 254], np.uint8),
        "u8_random": rng.integers(0, 256, (3, 1000)).astype(np.uint8),
        "i32_empty": np.zeros(0, np.int32),
        "i8_empty": np.zeros((0, 4), np.int8),
        "i32_all_equal": np.full(100, -77, np.int32),
        "u8_all_equal": np.full(100, 255, np.uint8),
        "i8_all_min": np.full(33, -128, np.int8),
    }


@pytest.mark.parametrize("name", list(arrays()))
def test_record_stats_is_the_numpy_of_the_definition(name):
    x = arrays()[name]
    s = tf.record_stats(x, name)
    assert s.name == name
    assert_is(s, x, name)


def test_bit_length_against_python_ints():
    x = arrays()["i32_extremes"]
    s = tf.record_stats(x)
    want = np.zeros(33, np.uint64)
    for v in x.tolist():
        want[abs(v).bit_length()] += 1
    assert np.array_equal(s.bits, want)
    assert s.bits[32] == 1 and s.bits[0] == 1
    assert s.absmax == 2 ** 31 and isinstance(s.absmax, int)
    assert tf.record_stats(np.array([3, -5], np.int8)).absmax == 5
    assert tf.record_stats(np.array([4, 6], np.int32)).mean == 5.0


def test_unsupported_dtypes_raise():
    for dt in (np.float32, np.int16, np.int64):
        with pytest.raises(ValueError):
            tf.record_stats(np.zeros(4, dt))


def test_merge_is_the_concatenation():
    a = arrays()
    for x, y in ((a["i32_random"], a["i32_extremes"]), (a["i8_random"], a["i8_extremes"]),
                 (a["u8_random"], a["u8_all_equal"])):
        m = tf.record_stats(x, "r").merge(tf.record_stats(y, "other"))
        assert m.name == "r"
        assert_is(m, np.concatenate([x.reshape(-1), y.reshape(-1)]))
    for key, empty in (("i32_random", "i32_empty"), ("i8_random", "i8_empty")):
        s, e = tf.record_stats(a[key]), tf.record_stats(a[empty])
        assert s.merge(e).equals(s) and e.merge(s).equals(s)
        assert e.merge(e).equals(tf.RecordStats.empty(s.dtype))
    with pytest.raises(ValueError):
        tf.record_stats(a["i8_random"]).merge(tf.record_stats(a["u8_random"]))
    with pytest.raises(ValueError):
        tf.record_stats(a["i32_random"]).merge(tf.record_stats(a["i8_random"]))


def test_sum_wraps_like_numpy_and_survives_json():
    big = tf.record_stats(np.full(1000, I32_MAX, np.int32), "big")
    s = big
    for _ in range(23):  # 2^23 x 1000 x (2^31 - 1) > 2^63: the sum wraps
        s = s.merge(s)
    n = 1000 * 2 ** 23
    want = (n * I32_MAX + 2 ** 63) % 2 ** 64 - 2 ** 63
    assert s.count == n and s.sum == want and abs(s.sum) > 2 ** 53
    back = tf.RecordStats.from_json(json.loads(json.dumps(s.to_json())))
    assert back.equals(s) and back.name == "big" and back.sum == want and back.count == n
    assert isinstance(s.to_json()["sum"], int) and all(isinstance(b, int) for b in s.to_json()["bits"])
    mid = tf.record_stats(np.full(3, I32_MAX, np.int32)).merge(tf.record_stats(np.full(3, I32_MIN, np.int32)))
    one = tf.RecordStats.from_json(json.loads(json.dumps(dict(mid.to_json(), sum=2 ** 53 + 1))))
    assert one.sum == 2 ** 53 + 1
    b8 = tf.record_stats(arrays()["i8_random"], "q")
    assert tf.RecordStats.from_json(json.loads(json.dumps(b8.to_json()))).equals(b8)


def test_bit_width_on_a_hand_made_histogram():
    bits = np.zeros(33, np.uint64)
    bits[0], bits[3], bits[7], bits[20] = 50, 940, 9, 1   # 1000 elements
    s = tf.RecordStats("h", "int32", 1000, 0, 2 ** 19, 0, bits, None)
    assert s.bit_width() == 20 and s.bit_width(1.0) == 20
    assert s.bit_width(0.99) == 3      # 990 of 1000 lie in bits[:4]
    assert s.bit_width(0.991) == 7
    assert s.bit_width(0.05) == 0
    signed = tf.RecordStats("h", "int32", 1000, -2 ** 19, 5, 0, bits, None)
    assert signed.bit_width() == 21 and signed.bit_width(0.99) == 4
    assert tf.RecordStats.empty("int8").bit_width() == 0
    x = np.array([-128, 5], np.int8)
    assert tf.record_stats(x).bit_width() == 9   # magnitude 128 takes 8 bits, plus the sign


@pytest.mark.parametrize("dtype", ["int8", "uint8"])
@pytest.mark.parametrize("q", [0, 0.5, 0.99999])
def test_percentile_abs_is_np_partition(dtype, q):
    rng = np.random.default_rng(11)
    info = np.iinfo(dtype)
    cases = [rng.integers(info.min, info.max + 1, 4001).astype(dtype),
             rng.integers(max(info.min, -3), 4, 257).astype(dtype),
             np.array([info.min, info.max, 0, 1], dtype),
             np.full(9, info.max, dtype)]
    for x in cases:
        k = int(x.size * q)
        assert tf.record_stats(x).percentile_abs(q) == int(np.partition(np.abs(x), k)[k])


def test_percentile_abs_needs_the_value_histogram():
    with pytest.raises(ValueError):
        tf.record_stats(np.arange(10, dtype=np.int32)).percentile_abs(0.5)
    with pytest.raises(ValueError):
        tf.RecordStats.empty("int8").percentile_abs(0.5)


@pytest.fixture(scope="module")
def lenet_files():
    """An unpacked and a packed trace of the oracle's LeNet-5 records (batch 3) plus a float record,
    and a second pair of other samples."""
    from oracle import graph_ref
    model = zoo.lenet5(batch=3)
    out = []
    for offset in (0, 3):
        recs = graph_ref.calibrate(model.mod, model.params, {"data": model.sample_inputs(offset, 3)}, threads=1)
        recs = {k: np.asarray(v) for k, v in recs.items()}
        recs["float_record"] = np.linspace(-1, 1, 12, dtype=np.float32).reshape(3, 4)
        v1 = tf.trace_bytes({"sample_offset": offset, "n_samples": 3}, {}, recs)
        out.append((recs, v1, tf.pack_trace(v1)))
    return out


def test_trace_stats_of_both_kinds_of_file(lenet_files):
    recs, v1, v2 = lenet_files[0]
    a, b = tf.trace_stats(v1), tf.trace_stats(v2)
    supported = [k for k, v in recs.items() if str(v.dtype) in ("int32", "int8", "uint8")]
    assert supported and list(a) == list(b) == supported
    assert "float_record" not in a
    assert {str(recs[k].dtype) for k in supported} >= {"int32", "int8"}
    for k in supported:
        assert a[k].equals(b[k]) and a[k].name == k
        assert_is(a[k], recs[k], k)


def test_stats_command_merges_files(lenet_files, tmp_path, capsys):
    paths = []
    for i, (_, v1, v2) in enumerate(lenet_files):
        p = tmp_path / f"f{i}.tkt"
        p.write_bytes(v2 if i else v1)   # one of each kind
        paths.append(str(p))
    assert tf.main(["stats"] + paths) == 0
    got = tf.stats_from_json(json.loads(capsys.readouterr().out))
    (r0, _, _), (r1, _, _) = lenet_files
    assert list(got) == [k for k in r0 if k != "float_record" and str(r0[k].dtype) in tf.STATS_KIND]
    for k, s in got.items():
        assert_is(s, np.concatenate([r0[k].reshape(-1), r1[k].reshape(-1)]), k)


class FakeTracer:
    """Writes chunk files of synthetic records; no statistics sidecars."""

    def __call__(self, offset, n, path):
        rng = np.random.default_rng(offset)
        recs = {"data": rng.integers(-128, 128, (n, 5)).astype(np.int8),
                "%0": rng.integers(I32_MIN, I32_MAX, (n, 7)).astype(np.int32),
                "%1": rng.standard_normal((n, 2)).astype(np.float32),
                "%2": rng.integers(0, 256, (n, 3)).astype(np.uint8)}
        with open(path, "wb") as f:
            f.write(tf.trace_bytes({"sample_offset": offset, "n_samples": n}, {}, recs))
        fut = concurrent.futures.Future()
        fut.set_result(tf.records_digest(recs))
        return fut


def test_merge_stats_reads_sidecars_and_falls_back(tmp_path):
    out = str(tmp_path)
    entries = trace_job.run(FakeTracer(), 10, 4, out)
    files = [str(tmp_path / e.file) for e in entries]
    assert len(files) == 3
    per_chunk = [tf.trace_stats(f) for f in files]
    for f, s in zip(files[:2], per_chunk[:2]):   # the third chunk has no sidecar
        trace_job.write_stats_file(trace_job.stats_file(f), s)
        assert not (tmp_path / (f + ".stats.json.tmp")).exists()
    logged = []
    merged = trace_job.merge_stats(out, 0, "trace", log=logged.append)
    assert len(logged) == 1 and "chunk 2" in logged[0]
    want = tf.merge_stats_dicts(per_chunk)
    assert list(merged) == ["data", "%0", "%2"]
    on_disk = trace_job.read_stats_file(str(tmp_path / "trace.rank0.stats.json"))
    for k in want:
        assert merged[k].equals(want[k]) and on_disk[k].equals(want[k]) and on_disk[k].name == k
    assert merged["%0"].count == 70 and merged["data"].count == 50
    # a sidecar is what the merge reads: a doctored one shows in the result
    doctored = dict(per_chunk[0])
    doctored["%2"] = doctored["%2"].merge(doctored["%2"])
    trace_job.write_stats_file(trace_job.stats_file(files[0]), doctored)
    again = trace_job.merge_stats(out, 0, "trace")
    assert again["%2"].count == want["%2"].count + per_chunk[0]["%2"].count
