"""tk_kl_candidates (csrc/tk_calibrate.cc): MinimizeKL's candidates one at a time, by the code
tk_find_scale_by_kl runs -- and the numpy model of the device search (tests/kl_cases.py) against
them: its intervals contain every host divergence, its survivors contain the host's argmin, and
the full-size cases stay within the cap of TK_KL_MAX_PICKS survivors by the model alone."""
import ctypes

import numpy as np
import pytest

from oracle import realize_ref
from tachikoma_amd import _lib
from tests import kl_cases as kc

SMALL = [s for s in kc.SHAPES if s not in kc.FULL]
HOST_OK = [c for c in kc.cases(SMALL) if c[3].max() <= kc.INT32_MAX]
FULL_OK = [c for c in kc.cases(kc.FULL) if c[3].max() <= kc.INT32_MAX]


def _ids(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize("label,bins,buckets,hist", HOST_OK + FULL_OK, ids=_ids(HOST_OK + FULL_OK))
def test_argmin_over_all_candidates_is_find_scale_by_kl(label, bins, buckets, hist):
    edges = kc.edges_of(bins)
    rows = kc.host_candidates(hist, bins, buckets)
    assert rows.size == kc.n_candidates(bins, buckets)
    k = kc.first_minimum(rows["div"])
    got = kc.edge_of(edges, bins, buckets, k)
    assert got.tobytes() == kc.host_threshold(hist, edges, bins, buckets).tobytes()


def test_divergences_choose_what_the_restatement_chooses():
    rng = np.random.default_rng(8)
    for dist in (rng.standard_normal(5000), np.abs(rng.standard_normal(5000)), rng.laplace(size=5000) * 3):
        arr = dist.astype(np.float32)
        thres = max(abs(arr.min()), abs(arr.max()))
        hist, edges = np.histogram(arr, bins=101, range=(-thres, thres))
        rows = kc.host_candidates(hist, 101, 11)
        k = kc.first_minimum(rows["div"])
        assert kc.edge_of(edges, 101, 11, k) == np.float32(realize_ref.minimize_kl(hist, edges, 101, 11))


@pytest.mark.parametrize("label,bins,buckets,hist", HOST_OK, ids=_ids(HOST_OK))
def test_subset_and_permutation_give_the_same_rows(label, bins, buckets, hist):
    rows = kc.host_candidates(hist, bins, buckets)
    n = rows.size
    order = np.random.default_rng(n).permutation(n)
    assert kc.host_candidates(hist, bins, buckets, order).tobytes() == rows[order].tobytes()
    some = order[::3]
    assert kc.host_candidates(hist, bins, buckets, some).tobytes() == rows[some].tobytes()
    twice = np.concatenate([some, some])
    assert kc.host_candidates(hist, bins, buckets, twice).tobytes() == rows[twice].tobytes()
    assert kc.host_candidates(hist, bins, buckets, np.zeros(0, np.int32)).size == 0


def test_refusals():
    lib = _lib.load()
    hist = np.ones(102, np.int32)
    cand = np.zeros(1, np.int32)
    out = np.zeros(1, kc.CAND_DTYPE)
    h = hist.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    c = cand.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    o = ctypes.c_void_p(out.ctypes.data)
    assert lib.tk_kl_candidates(h, 101, 11, c, 1, o) == 0
    for bins in (100, 102, 4):  # the window [zero - i, zero + i + 1) only fits an odd count
        assert lib.tk_kl_candidates(h, bins, 3, c, 1, o) == -1
        assert b"even" in lib.tk_last_error()
    assert lib.tk_kl_candidates(h, 101, 1, c, 1, o) == -1
    assert lib.tk_kl_candidates(h, 101, 102, c, 1, o) == -1
    assert lib.tk_kl_candidates(None, 101, 11, c, 1, o) == -1
    assert lib.tk_kl_candidates(h, 101, 11, None, 1, o) == -1
    assert lib.tk_kl_candidates(h, 101, 11, c, 1, None) == -1
    assert lib.tk_kl_candidates(h, 101, 11, c, -1, o) == -1
    for bad in (-1, kc.n_candidates(101, 11)):
        cand[0] = bad
        assert lib.tk_kl_candidates(h, 101, 11, c, 1, o) == -1
        assert b"outside" in lib.tk_last_error()


def _check_model(label, bins, buckets, hist, rows):
    host = kc.host_candidates(hist, bins, buckets)
    fin = np.isfinite(host["div"])
    # the exact parts: equality; +inf exactly where the host has it
    assert np.array_equal(np.isinf(rows["d"]), ~fin)
    for field in ("ps", "qs", "p_zeros", "q_zeros"):
        assert np.array_equal(rows[field], host[field]), field
    assert np.all(rows["bound"][~fin] == 0)
    err = np.abs(host["div"][fin].astype(np.float64) - rows["d"][fin])
    assert np.all(err <= rows["bound"][fin]), (label, float((err / rows["bound"][fin]).max()))
    status, keep = kc.survivors(hist, rows)
    if not fin.any():
        assert status == kc.ALL_INF
        return status, keep
    assert kc.first_minimum(host["div"]) in keep
    assert keep == sorted(keep)
    return status, keep


@pytest.mark.parametrize("label,bins,buckets,hist", HOST_OK, ids=_ids(HOST_OK))
def test_model_intervals_and_survivors(label, bins, buckets, hist):
    _check_model(label, bins, buckets, hist, kc.model(hist, bins, buckets))


@pytest.mark.parametrize("label,bins,buckets,hist", FULL_OK, ids=_ids(FULL_OK))
def test_model_full_size_stays_within_the_cap(label, bins, buckets, hist):
    status, keep = _check_model(label, bins, buckets, hist, kc.full_model(label, bins, buckets, hist))
    assert status == kc.FULL_STATUS[label.split("-")[0]]
    if status == kc.OK:
        assert 1 <= len(keep) <= kc.K


def test_model_reports_overflow():
    for label, bins, buckets, hist in kc.cases([(101, 11)]):
        if hist.max() > kc.INT32_MAX:
            assert kc.survivors(hist, np.zeros(0, kc.ROW_DTYPE)) == (kc.OVERFLOW, [])
