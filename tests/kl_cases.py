"""Cases and the numpy model for the kl_divergence threshold search on the device (csrc/tk_kl.hip).

Histograms are built directly as count arrays.  ``model`` is the statement of what the evaluate
kernel computes: per candidate, p, q, their smoothing, the sums ps / qs and the ratios in float32
exactly as the host's MinimizeKL has them (np.cumsum over float32 is the host's sequential sum),
then ``log`` and the running sum in float64, and beside it the bound of DESIGN.md section 2 on the
distance to the host's float32 divergence.  ``survivors`` is the select kernel."""
import ctypes

import numpy as np

from tachikoma_amd import _lib

F = np.float32
INT32_MAX = 2 ** 31 - 1
K = 32  # TK_KL_MAX_PICKS
OK, OVERFLOW, ALL_INF, TOO_MANY = 0, 1, 2, 3

SHAPES = [(3, 2), (11, 3), (101, 11), (255, 255), (257, 255), (1023, 2), (8001, 255), (8191, 511)]
FULL = [(8001, 255), (8191, 511)]

# the constants of csrc/tk_kl.h
U = 2.0 ** -24
HOST_LOG_ULPS = 2.0
TERM_REL = (2 * HOST_LOG_ULPS + 2) * U
TERM_ABS = 2.0 ** -149
ADD_REL = U + 2.0 ** -51
SLACK = 1 + 2.0 ** -30
EPS = F(0.0001)

CAND_DTYPE = np.dtype([("div", "<f4"), ("ps", "<f4"), ("qs", "<f4"), ("p_zeros", "<i4"), ("q_zeros", "<i4")])
ROW_DTYPE = np.dtype([("d", "<f8"), ("bound", "<f8"), ("ps", "<f4"), ("qs", "<f4"), ("p_zeros", "<i4"),
                      ("q_zeros", "<i4")])
PICK_DTYPE = np.dtype([("status", "<i4"), ("count", "<i4"), ("idx", "<i4", (K,))])


def n_candidates(bins, buckets):
    return bins // 2 + 1 - buckets // 2


# ---------------------------------------------------------------- histograms

def _bell(bins, total, seed):
    x = np.linspace(-4, 4, bins)
    w = np.exp(-0.5 * x * x)
    return np.random.default_rng(seed).poisson(w / w.sum() * total).astype(np.int64)


def gaussian(bins):
    return _bell(bins, 2_000_000, 1)


def relu(bins):
    """Post-ReLU: nothing below zero, half of the values in the centre bin."""
    h = _bell(bins, 1_000_000, 2)
    h[:bins // 2] = 0
    h[bins // 2] += 1_000_000
    return h


def sparse(bins):
    h = _bell(bins, 50_000_000, 3)
    keep = np.zeros(bins, bool)
    keep[bins // 2 % 50::50] = True  # the centre bin is one of them
    return np.where(keep, h, 0)


def extremes(bins):
    """Mass in the outermost bins only: a narrow window has an all-zero q and is +inf."""
    h = np.zeros(bins, np.int64)
    w = max(1, bins // 100)
    r = np.random.default_rng(4)
    h[:w] = r.integers(1, 5000, w)
    h[-w:] = r.integers(1, 5000, w)
    return h


def spike(bins):
    """One centre spike: q equals p in every window, every divergence is exactly 0."""
    h = np.zeros(bins, np.int64)
    h[bins // 2] = 123_457
    return h


def zeros(bins):
    return np.zeros(bins, np.int64)


def big(bins):
    """Counts of 2^24 + 1 and more in the tails and inside, so the float32 folds and sums round;
    the total stays below 2^31 (the host sums buckets in int)."""
    h = _bell(bins, 2_000_000, 5)
    vals = [2 ** 24 + 1, 2 ** 25 + 3, 2 ** 26 + 5, 2 ** 24 + 7, 2 ** 27 + 1, 2 ** 24 + 3]
    at = [0, 1 % bins, bins // 4, bins // 2, bins - 1 - bins // 4, bins - 1]
    for a, v in zip(at, vals):
        h[a] += v
    return h


def biggest(bins):
    """One count of almost INT32_MAX in the first bin; the total is INT32_MAX."""
    h = _bell(bins, 1000, 6)
    h[0] = 0
    h[0] = INT32_MAX - int(h.sum())
    return h


def over(bins):
    h = gaussian(bins)
    h[bins // 3] = 2 ** 31
    return h


KINDS = {"gaussian": gaussian, "relu": relu, "sparse": sparse, "extremes": extremes, "spike": spike, "zeros": zeros,
         "big": big, "biggest": biggest, "over": over}
# what the full-size records must come to by the model alone (the cap K is a condition): the spike
# is the exact tie of every candidate and therefore the too-many case, not a looseness of the bound
FULL_STATUS = {"gaussian": OK, "relu": OK, "sparse": OK, "extremes": OK, "big": OK, "biggest": OK, "spike": TOO_MANY,
               "zeros": ALL_INF, "over": OVERFLOW}


def cases(shapes=SHAPES):
    """[(label, bins, buckets, counts)]"""
    return [(f"{kind}-{bins}-{buckets}", bins, buckets, make(bins)) for bins, buckets in shapes
            for kind, make in KINDS.items()]


def edges_of(bins):
    return np.linspace(-3.0, 3.0, bins + 1).astype(F)


# ---------------------------------------------------------------- the host

def host_candidates(hist, bins, buckets, cand=None):
    """tk_kl_candidates' rows (CAND_DTYPE) for the listed candidates (default: all)."""
    cand = np.arange(n_candidates(bins, buckets), dtype=np.int32) if cand is None else np.ascontiguousarray(cand, np.int32)
    h = np.ascontiguousarray(hist, np.int32)
    out = np.zeros(cand.size, CAND_DTYPE)
    lib = _lib.load()
    assert lib.tk_kl_candidate_size() == CAND_DTYPE.itemsize
    _lib.check(lib.tk_kl_candidates(h.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), bins, buckets,
                                    cand.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), cand.size,
                                    ctypes.c_void_p(out.ctypes.data)), "tk_kl_candidates")
    return out


def host_threshold(hist, edges, bins, buckets):
    h = np.ascontiguousarray(hist, np.int32)
    e = np.ascontiguousarray(edges, F)
    out = ctypes.c_float()
    _lib.check(_lib.load().tk_find_scale_by_kl(h.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                               e.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), bins, buckets,
                                               ctypes.byref(out)), "tk_find_scale_by_kl")
    return F(out.value)


def edge_of(edges, bins, buckets, k):
    """The threshold of candidate k: its window's upper edge."""
    return F(edges[bins // 2 + buckets // 2 + k + 1])


# ---------------------------------------------------------------- the model of the evaluate kernel

def _wrap32(s):
    return (np.asarray(s, np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31


def _seq_sum(x):
    return np.cumsum(x, dtype=F)[-1] if x.size else F(0)


def _eps1(z, n):
    return F(F(EPS * F(z)) / F(n - z)) if n - z else F(0)


def model_candidate(hist, bins, buckets, k):
    """One ROW_DTYPE row.  ``hist``: int64 counts, none above INT32_MAX."""
    zero, i = bins // 2, buckets // 2 + k
    lo, hi = zero - i, zero + i + 1
    ln = hi - lo
    per = ln // buckets
    hf = hist.astype(F)
    win = hist[lo:hi].copy()
    win[0] = 0
    p = hf[lo:hi].copy()
    p[0] = _seq_sum(hf[:lo + 1])
    p[-1] = _seq_sum(hf[hi - 1:])
    bucket = np.minimum(np.arange(ln) // per, buckets - 1)
    merged = _wrap32(win[:buckets * per].reshape(buckets, per).sum(1)).astype(F)
    merged[-1] = F(merged[-1] + F(_wrap32(win[buckets * per:].sum())))
    nz = np.bincount(bucket, weights=win != 0, minlength=buckets).astype(np.int64)
    qb = np.where(nz > 0, merged / np.maximum(nz, 1).astype(F), F(0)).astype(F)
    q = np.where(p != 0, qb[bucket], F(0)).astype(F)
    zp, zq = int((p == 0).sum()), int((q == 0).sum())
    e1p, e1q = _eps1(zp, ln), _eps1(zq, ln)
    row = np.zeros((), ROW_DTYPE)
    row["p_zeros"], row["q_zeros"] = zp, zq
    if ln - zq == 0 or e1q >= 1:
        row["d"] = np.inf
        return row
    sp = np.where(p == 0, EPS, p - e1p).astype(F)
    sq = np.where(q == 0, EPS, q - e1q).astype(F)
    ps, qs = _seq_sum(sp), _seq_sum(sq)
    row["qs"] = qs
    if ln - zp == 0 or e1p >= 1:
        return row
    row["ps"] = ps
    pn, qn = (sp / ps).astype(F), (sq / qs).astype(F)
    use = (pn != 0) & (qn != 0)
    r = (pn[use] / qn[use]).astype(F)
    assert np.all(np.isfinite(r) & (r > 0))
    t = pn[use].astype(np.float64) * np.log(r.astype(np.float64))
    if t.size == 0:
        return row
    D = np.cumsum(t)
    # B_k = (B_{k-1} + tau_k)(1 + u) + ADD_REL |D_k|, unrolled
    g = (TERM_REL * np.abs(t) + TERM_ABS) * (1 + U) + ADD_REL * np.abs(D)
    B = float(np.sum(g * (1 + U) ** np.arange(t.size - 1, -1, -1)))
    row["d"], row["bound"] = D[-1], B * SLACK * (1 + 1e-12)  # the closed form rounds otherwise than the recurrence
    return row


def model(hist, bins, buckets, cand=None):
    """ROW_DTYPE rows of the listed candidates (default: all)."""
    cand = range(n_candidates(bins, buckets)) if cand is None else cand
    hist = np.asarray(hist, np.int64)
    assert hist.max(initial=0) <= INT32_MAX
    return np.array([model_candidate(hist, bins, buckets, int(k)) for k in cand], ROW_DTYPE)


def survivors(hist, rows):
    """The select kernel over a full table: (status, the survivors in ascending order)."""
    if np.asarray(hist).max(initial=0) > INT32_MAX:
        return OVERFLOW, []
    m = np.min(rows["d"] + rows["bound"])
    if m == np.inf:
        return ALL_INF, []
    keep = np.nonzero(rows["d"] - rows["bound"] <= m)[0]
    return (TOO_MANY if keep.size > K else OK), [int(k) for k in keep]


def first_minimum(div):
    """The host's argmin: strict <, so the first of equal minima."""
    return int(np.argmin(div))  # numpy's argmin takes the first too


_MODEL_CACHE = {}


def full_model(label, bins, buckets, hist):
    """The model over every candidate, computed once per case and shared by the tests."""
    if label not in _MODEL_CACHE:
        _MODEL_CACHE[label] = model(hist, bins, buckets)
    return _MODEL_CACHE[label]
