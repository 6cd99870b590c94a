"""The chain check on the MI355X (tk_check_chain, csrc/tk_chain.hip): every tail op of a fused
chain -- bias_add, requantize, [qnn.add], [clip] -- recomputed from its own recorded input and
compared with its recorded output, against oracle/qnn_ref.py.

Every chain here is built on the host: a conv record seeded over the whole int32 range, and the
records behind it computed by the oracle.  Such a chain is equal; a planted difference in one record
must show at that record's op with the exact count and first index, at the op that reads the record
only where the oracle says its result changes, and nowhere else.

The kernel's boundaries: a lane takes 4 elements, a step of the workgroup 1024, a workgroup
tk_chain_check_tile() = 4096; [3, 24, 9, 9] (5832 elements, 81-pixel planes) spans two workgroups
and has lanes whose elements cross a plane's end."""
import ctypes

import numpy as np
import pytest

from oracle import qnn_ref as ref
from tachikoma_amd import _lib
from tachikoma_amd.relay.build_module import requantize_plan

pytestmark = pytest.mark.gpu

NONE = _lib.NO_MISMATCH
CONV_BLOCK, DENSE_BLOCK, ADD_BLOCK = 13, 14, 15
SHAPES = [(3, 24, 9, 9), (2, 16, 7, 7), (2, 32, 1, 1), (3, 10), (1, 16, 16, 16)]
I32 = np.iinfo(np.int32)

# requantize cases: (name, per-axis scales?, rounding, scale ratio or None for random, per-axis zero points?)
RQ_CASES = {
    "identity": (False, "UPWARD", 1.0, False),
    "tensor_pow2": (False, "UPWARD", 0.5, False),
    "tensor_upward": (False, "UPWARD", None, True),
    "tensor_tonearest": (False, "TONEAREST", None, False),
    "axis_upward": (True, "UPWARD", None, True),
    "axis_tonearest": (True, "TONEAREST", None, True),
}
RQ_MODES = {"identity": 0, "tensor_pow2": 1, "tensor_upward": 2, "tensor_tonearest": 3, "axis_upward": 4,
            "axis_tonearest": 5}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Chain:
    """One conv / dense chain: host records by the oracle, device copies, the attrs."""

    def __init__(self, shape, dtype="int8", rq="axis_upward", clip=True, add=None, seed=0):
        rng = np.random.default_rng(seed)
        self.shape, self.dtype = shape, dtype
        C = shape[1]
        n = int(np.prod(shape))
        per_axis, rounding, ratio, axis_zp = RQ_CASES[rq]
        lo, hi = ref.dtype_range(dtype)
        out_scale = np.float32(0.05)
        # scales that bring the whole int32 range into a few times the 8-bit range: both saturations
        # and the values between occur
        if ratio is not None:
            in_scale = np.float32(out_scale * np.float32(ratio))
        elif per_axis:
            in_scale = (out_scale * rng.uniform(0.3, 3.0, C) * 2.0 ** -rng.integers(22, 27, C)).astype(np.float32)
        else:
            in_scale = np.float32(out_scale * 1.7 * 2.0 ** -23)
        izp = rng.integers(-1000, 1000, C).astype(np.int32) if axis_zp else np.int32(37)
        ozp = np.int32(-3 if dtype == "int8" else 120)
        conv = rng.integers(I32.min, I32.max, size=n, endpoint=True).astype(np.int32)
        if ratio is not None:
            # identity / power of two: values near the 8-bit range, or everything saturates
            conv = rng.integers(-200, 200, size=n).astype(np.int32)
        conv[:2] = [I32.min, I32.max]
        conv[-2:] = [I32.max, I32.min]
        conv = conv.reshape(shape)
        bias = rng.integers(I32.min, I32.max, size=C, endpoint=True).astype(np.int32) if ratio is None else \
            rng.integers(-50, 50, size=C).astype(np.int32)
        self.rq_args = dict(input_scale=in_scale, input_zero_point=izp, output_scale=out_scale, output_zero_point=ozp,
                            axis=1, rounding=rounding, out_dtype=dtype)
        self.bias = bias
        rec = [conv, ref.bias_add(conv, bias, 1)]
        rec.append(ref.requantize(rec[1], **self.rq_args))
        self.keep = []
        at = _lib.tk_block_attrs()
        mode, ms, ss = requantize_plan(in_scale, out_scale, rounding)
        assert mode == RQ_MODES[rq], (rq, mode)
        r = at.requantize
        r.mode, r.axis = mode, 1
        r.multiplier, r.shift = int(ms[0]), int(ss[0])
        if per_axis:
            r.multipliers, r.shifts = self._const(ms), self._const(ss)
        if axis_zp:
            r.input_zero_points = self._const(izp)
        else:
            r.input_zero_point = int(izp)
        r.output_zero_point = int(ozp)
        self.add_args = None
        if add is not None:
            block_is_rhs, s_blk, zp_blk, s_res, zp_res, s_out, zp_out = add
            res = rng.integers(lo, hi, size=shape, endpoint=True).astype(dtype)
            self.res = res
            sides = {"blk": (rec[2], np.float32(s_blk), np.int32(zp_blk)), "res": (res, np.float32(s_res), np.int32(zp_res))}
            lhs, rhs = (sides["res"], sides["blk"]) if block_is_rhs else (sides["blk"], sides["res"])
            self.add_args = dict(lhs_scale=lhs[1], lhs_zero_point=lhs[2], rhs_scale=rhs[1], rhs_zero_point=rhs[2],
                                 output_scale=np.float32(s_out), output_zero_point=np.int32(zp_out))
            self.block_is_rhs = block_is_rhs
            rec.append(self.add_of(rec[2]))
            at.has_add, at.block_is_rhs = 1, int(block_is_rhs)
            self.res_ref = _lib.TensorRef.from_torch(self._keep(_dev(res)))
            at.residual = self.res_ref.ptr
            for side, (_, s, zp) in (("lhs", lhs), ("rhs", rhs)):
                q = getattr(at.add, side)
                up = s.tobytes() == np.float32(s_out).tobytes() and int(zp) == int(zp_out)
                setattr(at.add, side + "_upcast", int(up))
                m, mm, sh = requantize_plan(s, np.float32(s_out), "UPWARD")
                q.mode, q.axis, q.multiplier, q.shift = m, -1, int(mm[0]), int(sh[0])
                q.input_zero_point, q.output_zero_point = int(zp), int(zp_out)
            at.add.output_zero_point = int(zp_out)
        self.clip_args = None
        if clip:
            self.clip_args = (float(lo + 40), float(hi - 30))
            rec.append(ref.clip(rec[-1], *self.clip_args))
            at.has_clip, at.clip_min, at.clip_max = 1, int(self.clip_args[0]), int(self.clip_args[1])
        self.attrs = at
        self.records = rec
        self.names = ["conv", "bias_add", "requantize"] + (["add"] if add is not None else []) + (["clip"] if clip else [])
        self.kind = CONV_BLOCK if len(shape) == 4 else DENSE_BLOCK
        self._dev = None

    @property
    def dev(self):
        """The records on the device (uploaded when first asked for)."""
        if self._dev is None:
            self._dev = [_dev(a) for a in self.records]
            self.bias_dev = _dev(self.bias)
        return self._dev

    def _keep(self, t):
        self.keep.append(t)
        return t

    def _const(self, a):
        return self._keep(_dev(np.asarray(a, np.int32))).data_ptr()

    def add_of(self, rq):
        a = self.add_args
        lhs, rhs = (self.res, rq) if self.block_is_rhs else (rq, self.res)
        return ref.qnn_add(lhs, rhs, a["lhs_scale"], a["lhs_zero_point"], a["rhs_scale"], a["rhs_zero_point"],
                           a["output_scale"], a["output_zero_point"])

    def check(self, tensors=None, bias=None, kind=None):
        """tk_check_chain on the device records: [(count, first)] per tail op."""
        tensors = self.dev if tensors is None else tensors
        self.dev  # (the bias)
        refs = [_lib.TensorRef.from_torch(t) for t in tensors]
        arr = (ctypes.POINTER(_lib.tk_tensor) * len(refs))(*[r.ptr for r in refs])
        b = _lib.TensorRef.from_torch(self.bias_dev if bias is None else bias)
        report = (_lib.tk_wire_mismatch * 8)()
        n = _lib.load().tk_check_chain(self.kind if kind is None else kind, arr, len(refs), b.ptr,
                                       ctypes.cast(ctypes.byref(self.attrs), ctypes.c_void_p), report, 8,
                                       ctypes.c_void_p(_lib.stream_handle()))
        _lib.check(min(n, 0), "tk_check_chain")
        assert n == len(refs) - 1
        return [(int(report[k].mismatches), int(report[k].first)) for k in range(n)]

    def planted(self, k, flats, delta=1):
        """Device records with record k changed at the flat indices ``flats``."""
        a = self.records[k].copy().reshape(-1)
        top = int(np.iinfo(a.dtype).max)
        for f in flats:
            v = int(a[f])
            a[f] = v - delta if v > top - delta else v + delta
        out = list(self.dev)
        out[k] = _dev(a.reshape(self.shape))
        return out, a.reshape(self.shape)


def _boundaries(shape):
    """Element 0, the last, both sides of every lane, step and workgroup boundary, and the first
    and last element of a channel plane (the second plane, the last plane)."""
    n = int(np.prod(shape))
    hw = int(np.prod(shape[2:]))
    tile = _lib.load().tk_chain_check_tile()
    assert tile == 4096
    pts = {0, n - 1, 3, 4, 1023, 1024, tile - 1, tile, hw - 1, hw, 2 * hw - 1, n - hw, n - hw - 1}
    return sorted(p for p in pts if 0 <= p < n)


# ---------------------------------------------------------------- equal chains
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("rq", sorted(RQ_CASES))
def test_equal_chains_report_nothing(device, shape, rq):
    for dtype, clip in (("int8", True), ("uint8", False)):
        ch = Chain(shape, dtype, rq, clip, seed=len(shape) + shape[1])
        assert ch.check() == [(0, NONE)] * (len(ch.records) - 1), (shape, rq, dtype)
    # the scales chosen do exercise the requantize: not everything saturates
    vals = np.unique(ch.records[2])
    assert len(vals) > 8


ADDS = {
    "lhs": (0, 0.05, -3, 0.03, 5, 0.06, 2),
    "rhs": (1, 0.05, -3, 0.03, 5, 0.06, 2),
    "block_upcast": (0, 0.05, -3, 0.02, 4, 0.05, -3),
    "residual_upcast_rhs": (1, 0.04, 1, 0.07, -6, 0.07, -6),
}


@pytest.mark.parametrize("shape", [(3, 24, 9, 9), (2, 32, 1, 1), (1, 16, 16, 16)], ids=str)
@pytest.mark.parametrize("add", sorted(ADDS))
def test_equal_chains_with_a_residual_add(device, shape, add):
    for dtype, clip in (("int8", True), ("uint8", True), ("int8", False)):
        cfg = list(ADDS[add])
        if dtype == "uint8":
            cfg[2], cfg[4], cfg[6] = cfg[2] + 128, cfg[4] + 128, cfg[6] + 128
        ch = Chain(shape, dtype, "axis_upward", clip, add=tuple(cfg), seed=7)
        assert bool(ch.attrs.add.lhs_upcast or ch.attrs.add.rhs_upcast) == ("upcast" in add)
        assert ch.check() == [(0, NONE)] * (len(ch.records) - 1), (shape, add, dtype, clip)
        assert len(np.unique(ch.records[3])) > 8


def test_add_block_chain(device):
    """The tail of an add block is its clip; an add block without a clip has no tail."""
    import torch
    rng = np.random.default_rng(5)
    for dtype in ("int8", "uint8"):
        lo, hi = ref.dtype_range(dtype)
        add = rng.integers(lo, hi, size=(3, 24, 9, 9), endpoint=True).astype(dtype)
        clip = ref.clip(add, lo + 50, hi - 20)
        at = _lib.tk_add_block_attrs()
        at.has_clip, at.clip_min, at.clip_max = 1, lo + 50, hi - 20
        bad = clip.copy().reshape(-1)
        where = [4095, 4096, 5831]
        bad[where] += 1
        for rec, want in ((clip, (0, NONE)), (bad.reshape(clip.shape), (3, 4095))):
            t = [_dev(add), _dev(rec)]
            refs = [_lib.TensorRef.from_torch(x) for x in t]
            arr = (ctypes.POINTER(_lib.tk_tensor) * 2)(*[r.ptr for r in refs])
            report = (_lib.tk_wire_mismatch * 2)()
            n = _lib.load().tk_check_chain(ADD_BLOCK, arr, 2, None, ctypes.cast(ctypes.byref(at), ctypes.c_void_p),
                                           report, 2, ctypes.c_void_p(_lib.stream_handle()))
            assert n == 1 and (int(report[0].mismatches), int(report[0].first)) == want
        at.has_clip = 0
        arr = (ctypes.POINTER(_lib.tk_tensor) * 1)(refs[0].ptr)
        assert _lib.load().tk_check_chain(ADD_BLOCK, arr, 1, None, ctypes.cast(ctypes.byref(at), ctypes.c_void_p),
                                          report, 2, ctypes.c_void_p(_lib.stream_handle())) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- planted differences
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_planted_differences_are_counted_and_located(device, shape):
    ch = Chain(shape, "int8", "axis_upward", True, add=ADDS["lhs"], seed=3)
    clean = [(0, NONE)] * 4
    assert ch.check() == clean
    pts = _boundaries(shape)
    # the clip record (nothing reads it): each point alone, then all of them at once
    k = ch.names.index("clip")
    for p in pts:
        got = ch.check(ch.planted(k, [p])[0])
        assert got == clean[:3] + [(1, p)], (p, got)
    got = ch.check(ch.planted(k, pts)[0])
    assert got == clean[:3] + [(len(pts), pts[0])]
    # the add record: its own op flags every point; the clip that reads it flags those where the
    # oracle's clip of the changed value is no longer the recorded clip
    k = ch.names.index("add")
    tensors, changed = ch.planted(k, pts)
    reclip = ref.clip(changed, *ch.clip_args).reshape(-1) != ch.records[k + 1].reshape(-1)
    want_clip = (int(reclip.sum()), int(np.flatnonzero(reclip)[0])) if reclip.any() else (0, NONE)
    assert ch.check(tensors) == clean[:2] + [(len(pts), pts[0]), want_clip]
    # the int32 conv record: only the bias_add op reads it
    for p in (pts[0], pts[-1], pts[len(pts) // 2]):
        assert ch.check(ch.planted(0, [p])[0]) == [(1, p)] + clean[1:], p
    assert ch.check(ch.planted(0, pts, delta=12345)[0]) == [(len(pts), pts[0])] + clean[1:]


@pytest.mark.parametrize("shape", [(3, 24, 9, 9), (3, 10)], ids=str)
@pytest.mark.parametrize("dtype", ["int8", "uint8"])
def test_the_ops_are_judged_independently(device, shape, dtype):
    """A difference in the bias_add record flags bias_add; requantize only where the oracle's
    requantize of the changed value differs from the recorded one; add and clip never."""
    ch = Chain(shape, dtype, "axis_upward", True, add=ADDS["rhs"] if dtype == "int8" else None, seed=11)
    n_tail = len(ch.records) - 1
    pts = _boundaries(shape)
    small, changed_small = ch.planted(1, pts, delta=1)
    big, changed_big = ch.planted(1, pts, delta=1 << 24)
    seen = set()
    for tensors, changed in ((small, changed_small), (big, changed_big)):
        rq = ref.requantize(changed, **ch.rq_args).reshape(-1) != ch.records[2].reshape(-1)
        want_rq = (int(rq.sum()), int(np.flatnonzero(rq)[0])) if rq.any() else (0, NONE)
        seen.add(bool(rq.any()))
        assert ch.check(tensors) == [(len(pts), pts[0]), want_rq] + [(0, NONE)] * (n_tail - 2)
    assert seen == {False, True}                       # one amount keeps the requantized values, one moves some
    # a requantize element changed: requantize and its reader, not bias_add
    tensors, changed = ch.planted(2, pts)
    nxt = (ch.add_of(changed) if ch.add_args else ref.clip(changed, *ch.clip_args)).reshape(-1) != ch.records[3].reshape(-1)
    want = (int(nxt.sum()), int(np.flatnonzero(nxt)[0])) if nxt.any() else (0, NONE)
    assert ch.check(tensors) == [(0, NONE), (len(pts), pts[0]), want] + [(0, NONE)] * (n_tail - 3)


def test_unaligned_buffers_take_the_narrow_path(device):
    """Records at addresses that allow neither 16-byte nor 4-byte loads: the same verdicts."""
    import torch
    ch = Chain((3, 24, 9, 9), "uint8", "tensor_tonearest", True, seed=2)
    n = ch.records[0].size
    pts = _boundaries(ch.shape)
    tensors, _ = ch.planted(3, pts)
    shifted = []
    for t in tensors:
        off = 1 if t.element_size() == 1 else 4 // t.element_size()      # 1 byte / 4 bytes past an aligned address
        buf = torch.empty(n + 16, dtype=t.dtype, device=t.device)
        view = buf[off:off + n].view(ch.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 != 0
        shifted.append(view)
    assert ch.check(shifted) == [(0, NONE), (0, NONE), (len(pts), pts[0])]


# ---------------------------------------------------------------- refusals
def test_refusals(device):
    import torch
    lib = _lib.load()
    ch = Chain((2, 16, 7, 7), "int8", "axis_upward", True, seed=1)
    s = ctypes.c_void_p(_lib.stream_handle())
    refs = [_lib.TensorRef.from_torch(t) for t in ch.dev]
    arr = (ctypes.POINTER(_lib.tk_tensor) * 4)(*[r.ptr for r in refs])
    bias = _lib.TensorRef.from_torch(ch.bias_dev)
    attrs = ctypes.cast(ctypes.byref(ch.attrs), ctypes.c_void_p)
    report = (_lib.tk_wire_mismatch * 4)()

    def call(kind=CONV_BLOCK, records=arr, n=4, b=bias.ptr, at=attrs, rep=report, cap=4):
        return lib.tk_check_chain(kind, records, n, b, at, rep, cap, s)

    assert call() == 3
    assert call(records=None) == -1 and b"null" in lib.tk_last_error()
    assert call(at=None) == -1
    assert call(rep=None) == -1
    assert call(b=None) == -1
    assert call(cap=2) == -1 and b"tail ops" in lib.tk_last_error()
    assert call(kind=7) == -1
    assert call(n=3) == -1                                   # has_clip says four records
    with_null = (ctypes.POINTER(_lib.tk_tensor) * 4)(refs[0].ptr, None, refs[2].ptr, refs[3].ptr)
    assert call(records=with_null) == -1
    # dtypes: an 8-bit conv record, an int32 requantize record, a clip of the other signedness
    for swap in ((0, 2), (2, 1)):
        r2 = list(refs)
        r2[swap[0]] = refs[swap[1]]
        assert call(records=(ctypes.POINTER(_lib.tk_tensor) * 4)(*[r.ptr for r in r2])) == -1, swap
    u8 = _lib.TensorRef.from_torch(ch.dev[3].view(torch.uint8))
    assert call(records=(ctypes.POINTER(_lib.tk_tensor) * 4)(refs[0].ptr, refs[1].ptr, refs[2].ptr, u8.ptr)) == -1
    assert b"dtype" in lib.tk_last_error()
    # a record of another shape; a bias of another length; a tensor with strides
    other = _lib.TensorRef.from_torch(torch.zeros((2, 16, 7, 8), dtype=torch.int8, device="cuda"))
    assert call(records=(ctypes.POINTER(_lib.tk_tensor) * 4)(refs[0].ptr, refs[1].ptr, refs[2].ptr, other.ptr)) == -1
    short = _lib.TensorRef.from_torch(ch.bias_dev[:8].contiguous())
    assert call(b=short.ptr) == -1
    strided = _lib.TensorRef.from_torch(ch.dev[3])
    st = (ctypes.c_int64 * 4)(784, 49, 7, 1)
    strided.struct.strides = ctypes.cast(st, ctypes.POINTER(ctypes.c_int64))
    assert call(records=(ctypes.POINTER(_lib.tk_tensor) * 4)(refs[0].ptr, refs[1].ptr, refs[2].ptr, strided.ptr)) == -1
    assert b"compact" in lib.tk_last_error()
    assert call() == 3 and all(r.mismatches == 0 for r in report[:3])
    torch.cuda.synchronize()
