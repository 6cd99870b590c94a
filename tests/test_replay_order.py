"""relay/replay.py: the schedule of a trace replay, on hand-written node_io tables.  Pure host
logic: neither torch nor the HIP library is involved."""
import pytest

from tachikoma_amd.relay.replay import UnsupportedError, replay_order, replay_units


def node(kind, records=(), reads=(), writes=(), shadows=None):
    return {"kind": kind, "records": list(records), "reads": list(reads),
            "writes": list(records) + [w for w in writes if w not in records], "shadows": dict(shadows or {})}


def epi(name):
    """writes / shadows of a node whose epilogue writes the shadow of its record ``name``."""
    return dict(writes=[f"shadow:{name}"], shadows={f"shadow:{name}": name})


def shadow_node(src):
    return node("shadow", [], [src], [f"shadow:{src}"], {f"shadow:{src}": src})


INPUTS = ["data"]

# data -> [shadow node] conv block a -> conv block b -> flatten -> dense (own shadow node)
CHAIN = [
    shadow_node("data"),
    node("conv_block", ["a0", "a1", "a2", "a3"], ["data", "shadow:data"], **epi("a3")),
    node("conv_block", ["b0", "b1", "b2"], ["a3", "shadow:a3"]),
    node("nn.batch_flatten", ["f"], ["b2"]),
    node("shadow", [], ["f"], ["shadow:d0:in"], {"shadow:d0:in": "f"}),
    node("conv_block", ["d0", "d1", "d2"], ["f", "shadow:d0:in"]),
]

# x -> p (3 records) ; x -> q (conv, bias, requantize, add, clip: the join sits in q's node and reads p2)
RESIDUAL = [
    shadow_node("data"),
    node("conv_block", ["x0", "x1", "x2", "x3"], ["data", "shadow:data"], **epi("x3")),
    node("conv_block", ["p0", "p1", "p2"], ["x3", "shadow:x3"]),
    node("conv_block", ["q0", "q1", "q2", "add", "clip"], ["x3", "shadow:x3", "p2"], **epi("clip")),
    node("nn.max_pool2d", ["pool"], ["clip", "shadow:clip"], **epi("pool")),
    node("conv_block", ["r0", "r1", "r2"], ["pool", "shadow:pool"]),
]

# a transposed (non-record) tensor "t:nchw_in" read by two convs through one shadow node, next to
# a record-sourced shadow (of data) written by a shadow node as well
SHARED_HELPER = [
    shadow_node("data"),
    node("conv_block", ["a0", "a1", "a2"], ["data", "shadow:data"]),
    node("transpose", [], ["a2"], ["t:nchw_in"]),
    shadow_node("t:nchw_in"),
    node("qnn.conv2d", ["c1"], ["t:nchw_in", "shadow:t:nchw_in"]),
    node("qnn.conv2d", ["c2"], ["t:nchw_in", "shadow:t:nchw_in"]),
    node("qnn.add", ["s"], ["c1", "c2"]),
]

# NHWC / HWIO conv: transpose in, [shadow], NCHW conv into scratch, transpose out = the record
LAYOUT = [
    node("qnn.quantize", ["q"], ["data"]),
    node("transpose", [], ["q"], ["c:nchw_in"]),
    shadow_node("c:nchw_in"),
    node("qnn.conv2d", [], ["c:nchw_in", "shadow:c:nchw_in"], ["c:nchw_out"]),
    node("transpose", ["c"], ["c:nchw_out"]),
    node("nn.bias_add", ["b"], ["c"]),
]

# BYOC composite: the contraction's accumulator is scratch, the post-ops write the one record
COMPOSITE = [
    shadow_node("data"),
    node("tachikoma.qnn.conv2d:contraction", [], ["data", "shadow:data"], ["k:acc"]),
    node("tachikoma.qnn.conv2d", ["k"], ["k:acc", "sum_in"]),
    node("cast", ["z"], ["k"]),
]

TABLES = {"chain": (CHAIN, INPUTS), "residual": (RESIDUAL, INPUTS), "shared_helper": (SHARED_HELPER, INPUTS),
          "layout": (LAYOUT, INPUTS), "composite": (COMPOSITE, ["data", "sum_in"])}


def simulate(node_io, inputs):
    """Run the order on flags.  Records start "recorded" (loaded from the file); a record node's
    writes turn its records "replayed".  Scratch is fresh only after the up-front rebuild or a
    write inside the unit that is running."""
    units, upfront = replay_units(node_io, inputs)
    order, upfront2 = replay_order(node_io, inputs)
    assert upfront2 == upfront and order == [i for u in reversed(units) for i in u]
    records = set(inputs) | {r for io in node_io for r in io["records"]}
    recorded = set(records)
    rebuilt = set(upfront)                   # up-front shadows that still hold the recorded tensor's
    ran = []
    for unit in reversed(units):
        assert unit == sorted(unit) and node_io[unit[-1]]["records"]
        assert all(not node_io[i]["records"] for i in unit[:-1])
        fresh = set()                        # what an earlier unit left in scratch does not count
        for i in unit:
            io = node_io[i]
            for b in io["reads"]:
                if b in records:
                    assert b in recorded, f"node {i} reads {b}, already replayed"
                else:
                    assert b in fresh or b in rebuilt, f"node {i} reads stale {b}"
            for b in io["writes"]:
                if b in records:
                    recorded.discard(b)
                elif io["records"]:
                    rebuilt.discard(b)       # an epilogue's shadow of a replayed record
                else:
                    fresh.add(b)
        ran.append(unit[-1])
    record_nodes = [i for i, io in enumerate(node_io) if io["records"]]
    assert ran == record_nodes[::-1]                         # every record node once, in reverse
    assert recorded == set(inputs)                           # graph inputs are loaded, never computed
    return units, upfront


@pytest.mark.parametrize("which", sorted(TABLES))
def test_order_reads_recorded_inputs_and_fresh_scratch(which):
    simulate(*TABLES[which])


def test_chain():
    order, upfront = replay_order(CHAIN, INPUTS)
    assert order == [5, 3, 2, 1]                             # the shadow nodes' work is done up front
    assert upfront == ["shadow:data", "shadow:a3", "shadow:d0:in"]


def test_residual_join_at_the_adds_position():
    units, upfront = replay_units(RESIDUAL, INPUTS)
    assert units == [[1], [2], [3], [4], [5]]
    assert replay_order(RESIDUAL, INPUTS)[0] == [5, 4, 3, 2, 1]   # q (reads p2) before p
    assert set(upfront) == {"shadow:data", "shadow:x3", "shadow:clip", "shadow:pool"}


def test_shared_helper_runs_in_both_units():
    units, upfront = replay_units(SHARED_HELPER, INPUTS)
    assert units == [[1], [2, 3, 4], [2, 3, 5], [6]]
    assert upfront == ["shadow:data"]                        # the record-sourced one only
    assert replay_order(SHARED_HELPER, INPUTS)[0] == [6, 2, 3, 5, 2, 3, 4, 1]


def test_layout_conv_with_its_transposes():
    units, upfront = replay_units(LAYOUT, INPUTS)
    assert units == [[0], [1, 2, 3, 4], [5]] and upfront == []


def test_composite_accumulator_is_scratch():
    units, upfront = replay_units(COMPOSITE, ["data", "sum_in"])
    assert units == [[1, 2], [3]] and upfront == ["shadow:data"]


def test_unwritten_scratch_is_refused_and_names_the_node():
    table = [node("qnn.quantize", ["q"], ["data"]),
             node("qnn.conv2d", ["c"], ["q", "c:nchw_in"])]     # nobody writes c:nchw_in
    with pytest.raises(UnsupportedError, match=r"node 1 \(qnn\.conv2d\).*c:nchw_in"):
        replay_order(table, INPUTS)
    # written, but only by a later node
    table.append(node("transpose", [], ["q"], ["c:nchw_in"]))
    with pytest.raises(UnsupportedError, match="node 1"):
        replay_order(table, INPUTS)
    # a helper's own missing input names the helper
    table = [node("transpose", [], ["ghost"], ["t"]), node("clip", ["c"], ["t"])]
    with pytest.raises(UnsupportedError, match=r"node 0 \(transpose\).*ghost"):
        replay_order(table, INPUTS)
    # without the graph inputs declared, reading one is such a read too
    with pytest.raises(UnsupportedError, match="data"):
        replay_order(CHAIN)


def test_unsupported_error_is_the_packages():
    from tachikoma_amd.relay.build_module import UnsupportedError as E
    assert E is UnsupportedError and issubclass(E, NotImplementedError)
