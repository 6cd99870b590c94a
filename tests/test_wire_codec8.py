"""1-byte records of the trace wire codec on the host (no GPU): plain and clamp-predicted records
round-trip bit-exactly through the reference encoder and the pool decoder, the encoded size is what
the format's rules say, int32 chains and clamp pairs share one buffer, and buffers or record lists
that do not parse are refused."""
import numpy as np
import pytest

from tachikoma_amd import _lib
from tests import wire_cases as wc
from tests import wire_cases8 as w8

LIB = _lib.load()
INVALID_ARG = -1   # TK_ERR_INVALID_ARG (include/tachikoma.h)
NAMES = {k: sorted(w8.contents(1, k, np.random.default_rng(0))) for k in w8.KINDS}
CASES = [(k, name) for k in w8.KINDS for name in NAMES[k]]


def _encode(records, diffs):
    offs, total = w8.layout(records)
    assert all(o % 2 == 1 for o in offs[:1])
    recs = w8.wire_records(records, diffs, offs)
    src = w8.image_of(records, offs, total)
    bound = LIB.tk_wire_bound(recs, len(records))
    assert bound > 0, LIB.tk_last_error()
    wire = np.zeros(bound, np.uint8)
    n = LIB.tk_wire_encode_host(recs, len(records), w8.ptr(src), total, w8.ptr(wire), bound)
    assert 0 < n <= bound, LIB.tk_last_error()
    return recs, src, wire, n, offs, total


def _decode(recs, records, wire, n, offs, total, threads=0):
    exact = np.ascontiguousarray(wire[:n]).copy()   # the wire bytes alone, in a buffer of that size
    out = w8.image_of([np.full_like(r, 0x3C) for r in records], offs, total)
    rc = LIB.tk_wire_decode(recs, len(records), w8.ptr(exact), n, w8.ptr(out), total, threads)
    return rc, out


@pytest.mark.parametrize("n", w8.SIZES)
@pytest.mark.parametrize("kind,name", CASES)
def test_roundtrip_is_bit_exact(kind, name, n):
    """Every content of both kinds on every size, records at odd image offsets with guard bytes
    between them: the decoded image equals the source image, the encoder's size and the widths it
    states are the ones the rules give (restated in NumPy), on one thread and on the pool."""
    records, diffs = w8.contents(n, kind, np.random.default_rng(n))[name]
    recs, src, wire, nbytes, offs, total = _encode(records, diffs)
    assert nbytes == w8.expected_bytes(records, diffs) == w8.parsed_bytes(wire, records)
    assert w8.stated_widths(wire, records) == w8.block_widths(records, diffs)
    for threads in (1, 0):
        rc, out = _decode(recs, records, wire, nbytes, offs, total, threads)
        assert rc == 0, LIB.tk_last_error()
        assert np.array_equal(out, src)


@pytest.mark.parametrize("kind", sorted(w8.KINDS))
def test_what_the_cases_cost(kind):
    """The cases do what they are named for: a clamp that holds costs no payload at all, an
    off-by-one element sends only its own block raw, a constant record is header only."""
    for n in w8.SIZES:
        c = w8.contents(n, kind, np.random.default_rng(n))
        for name in ("relu", "both_bounds", "identity", "dtype_ends", "block_unclamped") + \
                (("u8_above_127",) if kind == 2 else ()):
            records, diffs = c[name]
            assert set(w8.block_widths(records, diffs)[1]) == {0}, (name, n)
        records, diffs = c["off_by_one"]
        ws = w8.block_widths(records, diffs)[1]
        assert set(ws[:-1]) <= {0} and ws[-1] == (0 if (n - 1) % w8.BLOCK == 0 else 1), n
        assert set(w8.block_widths(*c["constant_plain"])[0]) == {0}
        assert set(w8.block_widths(*c["random_plain"])[0][:n // w8.BLOCK]) <= {1}   # the full blocks


def test_signed_compare_would_fail_the_uint8_case():
    """The uint8 case above 127 is one a signed compare gets wrong: restating the rule on the bytes
    viewed as int8 escapes blocks that the uint8 rule predicts."""
    records, diffs = w8.contents(3 * 256 + 17, 2, np.random.default_rng(4))["u8_above_127"]
    as_i8 = [r.view(np.int8) for r in records]
    assert set(w8.block_widths(records, diffs)[1]) == {0}
    assert 1 in w8.block_widths(as_i8, diffs)[1]


@pytest.mark.parametrize("kind", sorted(w8.KINDS))
@pytest.mark.parametrize("n", [257, 2 * w8.SEG + 300])
def test_int32_chain_and_clamp_pair_in_one_buffer(kind, n):
    """An int32 chain differenced twice, then a 1-byte record and its clamp, in one wire buffer."""
    rng = np.random.default_rng(n + kind)
    chain, cdiff = wc.contents(n, rng)["diff_chain"]
    pair, pdiff = w8.contents(n, kind, rng)["both_bounds"]
    records, diffs = chain + pair, cdiff + pdiff
    recs, src, wire, nbytes, offs, total = _encode(records, diffs)
    assert nbytes == w8.expected_bytes(records, diffs) == w8.parsed_bytes(wire, records)
    # against the int32 rules of tests/wire_cases.py: two buffers' sizes, less one 64-byte table line
    assert nbytes == wc.expected_bytes(chain, cdiff) + w8.expected_bytes(pair, pdiff) - 64
    for threads in (1, 0):
        rc, out = _decode(recs, records, wire, nbytes, offs, total, threads)
        assert rc == 0 and np.array_equal(out, src)


@pytest.mark.parametrize("kind", sorted(w8.KINDS))
def test_broken_buffers_and_record_lists_are_refused(kind):
    """A 1-byte segment that states width 2, a truncated buffer, and a clamp record whose
    predecessor has another size or kind all fail with TK_ERR_INVALID_ARG; the decoder is given
    exactly the bytes it may read."""
    n = 2 * w8.SEG + 300
    records, diffs = w8.contents(n, kind, np.random.default_rng(2))["both_bounds"]
    recs, src, wire, nbytes, offs, total = _encode(records, diffs)
    table = 64   # 6 segments

    def refused(w, nb):
        rc, _ = _decode(recs, records, w, nb, offs, total)
        return rc == INVALID_ARG
    assert refused(wire, 0) and refused(wire, table - 1) and refused(wire, table) and refused(wire, nbytes - 64)
    for seg in (0, 3):                                # a raw segment of the predecessor, a predicted one
        start = int(wire[4 * seg:4 * seg + 4].view(np.uint32)[0]) * 64
        bad = wire.copy()
        assert bad[table + start + 256 + 5] in (0, 1)
        bad[table + start + 256 + 5] = 2              # width of block 5 (64 blocks: 256 base bytes)
        assert refused(bad, nbytes)
    # every block of the predicted record claims a raw plane: longer than the buffer holds
    bad = wire.copy()
    for seg in (3, 4, 5):
        start = int(wire[4 * seg:4 * seg + 4].view(np.uint32)[0]) * 64
        nb = 64 if seg < 5 else 2
        bad[table + start + (4 * nb + 15) // 16 * 16:][:nb] = 1
    assert refused(bad, nbytes)
    # record lists: a predecessor of another size, of the other 1-byte kind, an int32 one, no predecessor
    for change in ("size", "kind", "int32", "first", "unknown"):
        r2 = w8.wire_records(records, diffs, offs)
        if change == "size":
            r2[0].n_elems -= 1
        elif change == "kind":
            r2[0].kind = 3 - kind
        elif change == "int32":
            r2[0].kind, r2[0].n_elems = 0, n // 4
        elif change == "first":
            r2[0].diff = 1
        else:
            r2[1].kind, r2[1].diff = 3, 0
        assert LIB.tk_wire_bound(r2, 2) == INVALID_ARG, change
        assert LIB.tk_wire_decode(r2, 2, w8.ptr(wire), nbytes, w8.ptr(src.copy()), total, 0) == INVALID_ARG, change
    # a record that does not fit the image
    r3 = w8.wire_records(records, diffs, offs)
    assert LIB.tk_wire_decode(r3, 2, w8.ptr(wire), nbytes, w8.ptr(src.copy()), offs[1] + n - 1, 0) == INVALID_ARG
    # the intact buffer still decodes
    rc, out = _decode(recs, records, wire, nbytes, offs, total)
    assert rc == 0 and np.array_equal(out, src)
