"""The residual join is fused into a conv block only where the MFMA conv kernels, the only ones
that have the join, take the conv: a conv of fewer than 16 output channels keeps its own block and
the add runs as an add block (it used to be fused and then refused at run time)."""
import pytest

from tachikoma_amd import relay, zoo
from tachikoma_amd.relay.build_module import exec_groups


def _pair(channels):
    b = zoo._Builder(12)
    shape = (3, channels, 9, 9)
    x = zoo._input(b, shape)
    p = zoo.conv_block(b, x, "p", channels, 3, pad=1, act=None)
    q = zoo.conv_block(b, x, "q", channels, 1, act=None)
    model = zoo._finish("pair", b, zoo.qadd(b, p, q, relu=True), shape, 12)
    return relay.build(model.mod, target="mi355x", params=model.params).plan


@pytest.mark.parametrize("channels,fused", [(8, False), (15, False), (16, True)])
def test_residual_add_is_absorbed_by_mfma_convs_only(channels, fused):
    groups = [(g.kind, [o.op for o in g.ops]) for g in exec_groups(_pair(channels))]
    block = ["qnn.conv2d", "nn.bias_add", "qnn.requantize"]
    if fused:
        assert groups == [("conv_block", block), ("conv_block", block + ["qnn.add", "clip"])]
    else:
        assert groups == [("conv_block", block), ("conv_block", block), ("add_block", ["qnn.add", "clip"])]
