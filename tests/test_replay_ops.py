"""relay/replay.py: attribute_ops, the one place where the replay compare (per node) and the chain
check (per tail op) become one verdict per op.  Hand-written node lists, no GPU."""
import ast
import os

from tachikoma_amd.relay.replay import attribute_ops

NONE = 0xFFFFFFFFFFFFFFFF
# a conv block with a residual add and a clip, an add block with a clip, a pool, a dense block
NODES = [(0, ["c", "c.bias", "c.rq", "c.add", "c.clip"]), (2, ["j", "j.clip"]), (3, ["pool"]),
         (5, ["fc", "fc.bias", "fc.rq"])]
TAILS = ["c.bias", "c.rq", "c.add", "c.clip", "j.clip", "fc.bias", "fc.rq"]


def _chain(**bad):
    out = {r: (0, NONE) for r in TAILS}
    out.update(bad)
    return out


def _brief(ops):
    return [(o["name"], o["node"], o["place"], o["basis"], o["count"], o["first"]) for o in ops]


def test_clean():
    assert attribute_ops(NODES, {}, _chain()) == []
    assert attribute_ops(NODES, {"c": (0, NONE)}, _chain()) == []       # equal records may be listed with no count
    assert attribute_ops([], {}, {}) == []


def test_head_only():
    """The head differs and nothing behind it does (the difference did not survive the requantize)."""
    ops = attribute_ops(NODES, {"fc": (2, 7)}, _chain())
    assert _brief(ops) == [("fc", 5, 0, "node", 2, 7)]


def test_tail_only():
    """A tail record that is not its op of its input: the replay lists it, the verdict is the chain check's."""
    ops = attribute_ops(NODES, {"c.rq": (1, 40), "c.add": (1, 40)}, _chain(**{"c.rq": (1, 40)}))
    assert _brief(ops) == [("c.rq", 0, 2, "input", 1, 40)]
    # count and index are the chain check's, not the replay's
    ops = attribute_ops(NODES, {"j.clip": (9, 1)}, _chain(**{"j.clip": (3, 5)}))
    assert _brief(ops) == [("j.clip", 2, 1, "input", 3, 5)]


def test_head_with_a_consistent_tail():
    """A producer's wrong convolution, carried on consistently: every record of the node differs in
    the replay, the conv alone is faulty."""
    mism = {r: (1, 11) for r in NODES[0][1]}
    assert _brief(attribute_ops(NODES, mism, _chain())) == [("c", 0, 0, "node", 1, 11)]


def test_two_faults_in_one_chain():
    mism = {"c": (1, 3), "c.bias": (1, 3), "c.clip": (1, 90)}
    ops = attribute_ops(NODES, mism, _chain(**{"c.clip": (1, 90)}))
    assert _brief(ops) == [("c", 0, 0, "node", 1, 3), ("c.clip", 0, 4, "input", 1, 90)]
    # a corrupted record in the middle: its producer's fault and its consumer's
    ops = attribute_ops(NODES, {"c.rq": (1, 8)}, _chain(**{"c.rq": (1, 8), "c.add": (1, 8)}))
    assert [(o["name"], o["basis"]) for o in ops] == [("c.rq", "input"), ("c.add", "input")]


def test_faults_in_several_nodes_come_in_node_then_chain_order():
    mism = {"fc.rq": (1, 0), "pool": (4, 2), "c.bias": (1, 1)}
    ops = attribute_ops(NODES, mism, _chain(**{"fc.rq": (1, 0), "c.bias": (1, 1)}))
    assert [o["name"] for o in ops] == ["c.bias", "pool", "fc.rq"]
    assert [o["basis"] for o in ops] == ["input", "node", "input"]


def test_single_record_node():
    assert _brief(attribute_ops(NODES, {"pool": (4, 2)}, _chain())) == [("pool", 3, 0, "node", 4, 2)]
    # also when no chain check was made at all
    assert _brief(attribute_ops([(3, ["pool"])], {"pool": (4, 2)}, None)) == [("pool", 3, 0, "node", 4, 2)]


def test_a_graph_input_is_never_listed():
    """Graph inputs are loaded, not computed: no node writes them, so they cannot be an op."""
    assert attribute_ops(NODES, {"data": (5, 0)}, _chain()) == []
    ops = attribute_ops(NODES, {"data": (5, 0), "pool": (1, 1)}, _chain(**{"data": (5, 0)}))
    assert [o["name"] for o in ops] == ["pool"]


def test_a_chain_the_check_does_not_cover_keeps_node_granularity():
    """No chain verdicts for a node's tail (no check made, or its kind is not in the table): the
    node's first differing record stands for it, as FaultyNode.first does."""
    mism = {"c.bias": (2, 6), "c.rq": (2, 6), "fc": (1, 0), "fc.rq": (1, 0)}
    ops = attribute_ops(NODES, mism, None)
    assert _brief(ops) == [("c.bias", 0, 1, "node", 2, 6), ("fc", 5, 0, "node", 1, 0)]
    partial = {r: (0, NONE) for r in TAILS if not r.startswith("c.")}
    partial["fc.rq"] = (1, 0)
    ops = attribute_ops(NODES, mism, partial)
    assert _brief(ops) == [("c.bias", 0, 1, "node", 2, 6), ("fc", 5, 0, "node", 1, 0), ("fc.rq", 5, 2, "input", 1, 0)]


def test_replay_module_needs_the_standard_library_only():
    import tachikoma_amd.relay.replay as mod
    tree = ast.parse(open(mod.__file__).read())
    imported = {a.name.split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    imported |= {n.module.split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.module}
    assert imported <= {"__future__", "typing"}, imported
    assert os.path.basename(mod.__file__) == "replay.py"
