"""tk_conv2d_make_shadow_batch on the MI355X: the shadows of a mixed list of tensors in one launch,
against a NumPy restatement of the layout and against tk_conv2d_make_shadow on the same tensors."""
import ctypes

import numpy as np
import pytest

from tachikoma_amd import _lib

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 64

# (N, C, H, W), dtype
SHAPES = [
    ((1, 3, 5, 5), "int8"),      # fewer than 16 channels, odd plane
    ((2, 16, 1, 1), "uint8"),    # HW = 1
    ((3, 17, 7, 7), "int8"),     # one real channel in the last chunk; every plane after the first unaligned
    ((2, 40, 9, 9), "uint8"),
    ((2, 32, 4, 8), "int8"),     # everything 16-byte aligned: the wide path alone
    ((1, 16, 16, 17), "uint8"),  # more than one 256-pixel tile, a ragged last one
    ((1, 64, 14, 14), "int8"),
]


def layout(x: np.ndarray) -> np.ndarray:
    """The shadow of NCHW 8-bit ``x``, flat: [ceil(C/16)][N*H*W][16] bytes, byte (k, n*HW + p, j) =
    channel 16k + j of pixel p of image n, 0 for a channel >= C, uint8 data xor 0x80."""
    n, c, h, w = x.shape
    hw, chunks = h * w, (c + 15) // 16
    b = x.reshape(n, c, hw).view(np.uint8)
    if x.dtype == np.uint8:
        b = b ^ np.uint8(0x80)
    out = np.zeros((chunks, n * hw, 16), np.uint8)
    for ch in range(c):
        out[ch // 16, :, ch % 16] = b[:, ch, :].reshape(-1)
    return out.reshape(-1)


def _rand(rng, shape, dtype):
    info = np.iinfo(dtype)
    return rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dtype)


class Case:
    """Tensors on the device, each ``shift`` bytes into an allocation of its own, and a prefilled
    shadow with a guard region behind it for each."""

    def __init__(self, specs, shift=0, seed=0):
        import torch
        rng = np.random.default_rng(seed)
        self.lib = _lib.load()
        self.host = [_rand(rng, s, d) for s, d in specs]
        self.src, self.refs, self.sizes = [], [], []
        for x in self.host:
            t = torch.zeros(x.nbytes + 32, dtype=torch.uint8, device="cuda")
            t[shift:shift + x.nbytes] = torch.from_numpy(x.reshape(-1).view(np.uint8).copy()).cuda()
            self.src.append(t)
            self.refs.append(_lib.TensorRef(t.data_ptr() + shift, x.shape, str(x.dtype)))
            self.sizes.append(int(self.lib.tk_conv2d_shadow_bytes(self.refs[-1].ptr)))
        assert self.sizes == [layout(x).size for x in self.host]
        self.stream = ctypes.c_void_p(_lib.stream_handle(None))

    def shadows(self):
        import torch
        out = [torch.full((n + GUARD,), FILL, dtype=torch.uint8, device="cuda") for n in self.sizes]
        assert all(t.data_ptr() % 16 == 0 for t in out)
        return out

    def batch(self):
        out = self.shadows()
        n = len(out)
        data = (ctypes.POINTER(_lib.tk_tensor) * max(1, n))(*[r.ptr for r in self.refs])
        dst = (ctypes.c_void_p * max(1, n))(*[t.data_ptr() for t in out])
        rc = self.lib.tk_conv2d_make_shadow_batch(data, dst, n, self.stream)
        assert rc == 0, self.lib.tk_last_error()
        return [t.cpu().numpy() for t in out]

    def single(self):
        out = self.shadows()
        for r, t in zip(self.refs, out):
            assert self.lib.tk_conv2d_make_shadow(r.ptr, ctypes.c_void_p(t.data_ptr()), self.stream) == 0
        return [t.cpu().numpy() for t in out]

    def check(self):
        got, one = self.batch(), self.single()
        for i, (x, g, o, n) in enumerate(zip(self.host, got, one, self.sizes)):
            what = f"tensor {i} {x.shape} {x.dtype}"
            np.testing.assert_array_equal(g[:n], layout(x), err_msg=what)
            np.testing.assert_array_equal(g[:n], o[:n], err_msg=what + " vs tk_conv2d_make_shadow")
            assert (g[n:] == FILL).all(), what + ": the guard behind the shadow was written"


def test_mixed_list(device):
    Case(SHAPES).check()


def test_each_alone(device):
    for spec in SHAPES:
        Case([spec], seed=1).check()


@pytest.mark.parametrize("shift", [1, 4, 7])
def test_sources_off_alignment(device, shift):
    Case(SHAPES, shift=shift, seed=shift).check()


def test_same_list_again_with_new_contents(device):
    """The item table is kept per list of tensors: a second call reads the tensors anew."""
    import torch
    c = Case(SHAPES, seed=2)
    c.check()
    rng = np.random.default_rng(3)
    out = c.shadows()
    n = len(out)
    data = (ctypes.POINTER(_lib.tk_tensor) * n)(*[r.ptr for r in c.refs])
    dst = (ctypes.c_void_p * n)(*[t.data_ptr() for t in out])
    for _ in range(2):
        c.host = [_rand(rng, x.shape, x.dtype) for x in c.host]
        for t, x in zip(c.src, c.host):
            t[:x.nbytes] = torch.from_numpy(x.reshape(-1).view(np.uint8).copy()).cuda()
        assert c.lib.tk_conv2d_make_shadow_batch(data, dst, n, c.stream) == 0, c.lib.tk_last_error()
        for x, t, size in zip(c.host, out, c.sizes):
            g = t.cpu().numpy()
            np.testing.assert_array_equal(g[:size], layout(x))
            assert (g[size:] == FILL).all()


def test_seventy_tiny_tensors(device):
    rng = np.random.default_rng(4)
    specs = [((int(rng.integers(1, 3)), int(rng.integers(1, 20)), int(rng.integers(1, 4)), int(rng.integers(1, 4))),
              "int8" if i % 2 else "uint8") for i in range(70)]
    Case(specs, seed=5).check()


def test_empty_list_and_refusals(device):
    import torch
    lib = _lib.load()
    s = ctypes.c_void_p(_lib.stream_handle(None))
    assert lib.tk_conv2d_make_shadow_batch(None, None, 0, s) == 0          # n = 0: nothing to do
    c = Case(SHAPES[:2], seed=6)
    out = c.shadows()
    PT = ctypes.POINTER(_lib.tk_tensor)

    def call(refs=None, dsts=None, n=2, data_null=False, dst_null=False):
        refs = [r.ptr for r in c.refs] if refs is None else refs
        dsts = [t.data_ptr() for t in out] if dsts is None else dsts
        data = None if data_null else (PT * 2)(*refs)
        dst = None if dst_null else (ctypes.c_void_p * 2)(*dsts)
        return lib.tk_conv2d_make_shadow_batch(data, dst, n, s)

    assert call(data_null=True) == -1 and call(dst_null=True) == -1 and call(n=-1) == -1
    assert call(refs=[c.refs[0].ptr, PT()]) == -1                            # a null tensor
    assert call(dsts=[out[0].data_ptr(), None]) == -1                        # a null shadow
    assert call(dsts=[out[0].data_ptr(), out[1].data_ptr() + 8]) == -1       # not 16-byte aligned
    x3 = _lib.TensorRef(c.src[1].data_ptr(), (2, 16, 1), "int8")
    i32 = _lib.TensorRef(c.src[1].data_ptr(), (1, 2, 2, 2), "int32")
    f32 = _lib.TensorRef(c.src[1].data_ptr(), (1, 2, 2, 2), "float32")
    for bad in (x3, i32, f32):
        assert call(refs=[c.refs[0].ptr, bad.ptr]) == -1                     # not 4-D 8-bit
        assert b"make_shadow_batch" in lib.tk_last_error()
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == FILL).all() for t in out)                 # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
