"""The fused block kernels over every requantize mode and value range (tests/block_value_cases.py)
against the CPU oracle, bit for bit: each geometry is the smallest shape at which one kernel family
is still listed, each regime keeps most requantize outputs unsaturated (test_block_value_cases.py
proves that of the reference alone), and every kernel the block lists for the case's attrs runs.
"""
import re

import numpy as np
import pytest

from tests import block_value_cases as bvc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tk(device):
    from tests import tk_gpu
    return tk_gpu


def _conv_kw(c):
    g = c.geom
    kw = dict(clip=g.clip, out_dtype=g.dtype, want_shadow=True, poison=True, rounding=c.rounding, rq_zp=c.rq_zp,
              zw_vec=c.zw_vec, **g.conv_kw)
    if c.residual is not None:
        kw.update(residual=c.residual, add_params=c.add_params, block_is_rhs=g.block_is_rhs)
    return kw


def _run(tk, c, algo=0, **extra):
    g = c.geom
    if g.dense:
        return tk.dense_block(c.x, c.w, c.bias, g.za, g.zw, c.s_in, bvc.S_OUT, g.zp_out, clip=g.clip, rq_zp=c.rq_zp,
                              rounding=c.rounding, out_dtype=g.dtype)
    return tk.conv2d_block(c.x, c.w, c.bias, g.za, g.zw, c.s_in, bvc.S_OUT, g.zp_out, algo=algo, **_conv_kw(c), **extra)


def _listed(tk, c):
    """(algo, description) of every kernel the block lists for this case's attrs; none for the
    depthwise, direct and dense blocks, which have a single kernel."""
    return [] if c.geom.dense else _run(tk, c, algos_only=True, algo_info=True)


@pytest.mark.parametrize("name,regime,mode", bvc.CASE_IDS, ids=["-".join(i) for i in bvc.CASE_IDS])
def test_block_values(tk, name, regime, mode):
    """Every record and the shadow of the block, on the library's choice (algo 0) and on each
    listed kernel, equal the oracle's."""
    c = bvc.build(name, regime, mode)
    exp = c.expected + ([c.shadow] if c.shadow is not None else [])
    what = ["conv", "bias_add", "requantize"] + (["add"] if c.residual is not None else []) + ["clip"]
    what += ["shadow"] if c.shadow is not None else []
    bad = []
    for algo, desc in [(0, "the library's choice")] + _listed(tk, c):
        outs = _run(tk, c, algo=algo)
        assert len(outs) == len(exp)
        for label, got, e in zip(what, outs, exp):
            assert got.shape == e.shape and got.dtype == e.dtype, (algo, label, got.shape, got.dtype)
            if not np.array_equal(got, e):
                where = np.argwhere(got != e)
                first = tuple(where[0].tolist())
                bad.append(f"algo {algo} ({desc}) {label}: {len(where)} of {e.size} differ, first at {list(first)} "
                           f"({got[first]} for {e[first]}), "
                           f"index ranges {where.min(0).tolist()}..{where.max(0).tolist()}")
    assert not bad, "\n".join(bad)


def test_every_family_is_covered(tk):
    """The geometry list still reaches every kernel family: im2col tiles (1), both persistent
    algos (3, 4), the dense tile kernel (5), image-tile plans of 32 and 64 rows, of 32-, 64- and
    128-channel stages, a split-K plan and a plan with several images per workgroup; the
    depthwise, direct and dense blocks have their single kernel."""
    algos, descs, single = set(), [], []
    for g in bvc.GEOMETRIES:
        for regime, mode in (("calibrated", "AXIS_UPWARD"), ("calibrated", "AXIS_TONEAREST")):
            listed = _listed(tk, bvc.build(g.name, regime, mode))
            algos |= {a for a, _ in listed}
            descs += [d for a, d in listed if a >= 16]
            if not listed and mode == "AXIS_UPWARD":
                single.append(g.name)
    assert {1, 3, 4, 5} <= algos, sorted(algos)
    img = [d for d in descs if d.startswith("image tiles")]
    assert img, descs[:10]
    heads = [d.split("; split K")[0] for d in img]  # the plan itself, without its split-K epilogue pass
    for pattern in (r": 32 rows x", r": 64 rows x", r" 32-channel stages", r" 64-channel stages",
                    r" 128-channel stages", r"rows x ([2-9]|[1-9][0-9]+) images "):
        assert any(re.search(pattern, d) for d in heads), (pattern, sorted(set(heads))[:40])
    assert any("; split K" in d for d in img), sorted(set(img))[:40]
    assert sorted(single) == sorted(g.name for g in bvc.GEOMETRIES if g.dense or g.groups > 1 or g.name == "direct_5x5")
