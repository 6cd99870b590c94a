"""GraphModule.replay_trace at op granularity on the MI355X: the chain check
(tk_module_check_chains) between the store pass and the node run gives every tail op of a fused
node its own verdict, relay/replay.py: attribute_ops joins it with the node replay's.

The graphs are those of tests/test_gpu_trace_replay.py; as there, the module runs another input
before every replay.  Faults are planted in the version-1 file on the host, with the records behind
them recomputed by the oracle (oracle/graph_ref.py: eval_call) where the test wants a consistent
chain, and the packed file is derived with pack_trace."""
import json
import os
import shutil

import numpy as np
import pytest

from oracle import graph_ref
from tachikoma_amd import _lib, relay, trace_job, zoo
from tachikoma_amd import trace_format as tf
from tachikoma_amd.contrib import graph_executor
from tests.test_gpu_trace_replay import _node_of, _pad24, _run_b

pytestmark = pytest.mark.gpu

MODELS = {
    "lenet5_b3": lambda: (zoo.lenet5(batch=3), 3),
    "resnet18": lambda: (zoo.resnet18(batch=2, hw=32), 2),
    "resnet50": lambda: (zoo.resnet50(batch=2, hw=32), 2),
    "mobilenet_v2": lambda: (zoo.mobilenet_v2(batch=2, hw=32), 2),
    "pad24": lambda: (_pad24(), 3),
}


class Graph:
    def __init__(self, which):
        import tempfile
        self.model, batch = MODELS[which]()
        lib = relay.build(self.model.mod, target="mi355x", params=self.model.params)
        self.gm = graph_executor.GraphModule(lib["default"]())
        self.a = {self.model.input_name: self.model.sample_inputs(0, batch)}
        self.b = {self.model.input_name: self.model.sample_inputs(batch, batch)}
        self.gm.set_input(**self.a)
        with tempfile.TemporaryDirectory() as d:
            p1, p2 = os.path.join(d, "a.plain.tkt"), os.path.join(d, "a.packed.tkt")
            self.gm.dump_trace(p1)
            self.gm.dump_trace(p2, packed=True)
            self.files = (open(p1, "rb").read(), open(p2, "rb").read())
        self.records = {k: v.copy() for k, v in tf.read_trace(self.files[0]).records.items()}
        # the Relay call of every op record, named as Trace.calibrate names them
        self.calls, n = {}, 0
        func = self.model.mod["main"]
        for node in graph_ref._post_order(func.body):
            if type(node).__name__ == "Call" and not (node.op == "reshape" and type(node.args[0]).__name__ == "Constant"):
                self.calls[f"%{n}"] = node
                n += 1
        self.names = {id(c): k for k, c in self.calls.items()}
        self.node_of = _node_of(self.gm)
        self.ops = {o.name: o.op for o in self.gm.plan.ops}

    def eval(self, name, records):
        """The oracle's value of op record ``name`` from the records ``records`` of its arguments."""
        call = self.calls[name]

        def value(e):
            kind = type(e).__name__
            if kind == "Var":
                return np.asarray(self.model.params[e.name_hint]) if e.name_hint in self.model.params else records[e.name_hint]
            if kind == "Constant":
                return e.data
            return records[self.names[id(e)]]
        return graph_ref.eval_call(call, [value(e) for e in call.args])

    def rewritten(self, new):
        """The version-1 file with the records ``new`` ({name: array}) replaced, and its packed form."""
        recs = [(t.name, t.shape, t.dtype) for t in self.gm.plan.records]
        blob = bytearray(self.files[0])
        ct = tf.check_trace(bytes(blob), recs)
        for name, arr in new.items():
            e = next(e for e in ct.entries if e.name == name)
            raw = np.ascontiguousarray(arr).tobytes()
            assert len(raw) == e.raw_size and str(arr.dtype) == e.dtype
            at = ct.records_off + e.raw_off
            blob[at:at + len(raw)] = raw
        return bytes(blob), tf.pack_trace(bytes(blob))

    def chains(self, min_records=4):
        """(node, records) of the conv blocks with at least ``min_records`` records, in node order."""
        mod = self.gm.module
        return [(i, recs) for i, (k, recs) in enumerate(zip(mod.node_kinds, mod.node_records))
                if k == "conv_block" and len(recs) >= min_records]


@pytest.fixture(scope="module")
def graphs():
    built = {}

    def get(which):
        if which not in built:
            built[which] = Graph(which)
        return built[which]

    yield get
    for g in built.values():
        g.gm.close()
    import gc
    gc.collect()


def _bump(a, flat, delta=1):
    """A copy of ``a`` with element ``flat`` moved by ``delta`` (downwards where it would overflow)."""
    out = a.copy()
    top = int(np.iinfo(a.dtype).max)
    v = int(out.reshape(-1)[flat])
    out.reshape(-1)[flat] = v - delta if v > top - delta else v + delta
    return out


def _brief(ops):
    return [(o.name, o.basis, o.count, o.flat_index) for o in ops]


def _consistent(rep):
    """What must hold for every report: ok == (not ops) (the params are equal in these tests), the
    ops grouped per node are the ops, and an op's record is one of its node's."""
    assert rep.params_equal and rep.ok == (not rep.ops), rep
    assert sorted((o.name for n in rep.nodes for o in n.ops)) == sorted(o.name for o in rep.ops)
    for n in rep.nodes:
        assert all(o.node == n.node and n.records[o.place] == o.name for o in n.ops)
        assert n.ops, n                                         # a faulty node has a faulty op
    assert {o.node for o in rep.ops} == {n.node for n in rep.nodes}


# ---------------------------------------------------------------- clean files
@pytest.mark.parametrize("which", sorted(MODELS))
def test_clean_files_have_no_faulty_op(device, graphs, which):
    import torch
    g = graphs(which)
    gm = g.gm
    tails = [r for k, recs in zip(gm.module.node_kinds, gm.module.node_records)
             if k in ("conv_block", "dense_block", "add_block") for r in recs[1:]]
    assert gm.module.chain_ops() == tails and tails
    for blob in g.files:
        _run_b(gm, g.b)
        rep = gm.replay_trace(blob)
        assert rep.ok and rep.ops == [] and rep.nodes == [] and rep.mismatches == [], (which, rep)
        assert rep.stats["chain_ms"] >= 0
        _consistent(rep)
        # the chain check on loaded data: every fused epilogue is bit for bit its per-op semantics
        _run_b(gm, g.b)
        gm.load_trace(blob)
        found = gm.module.check_chains(torch.cuda.current_stream())
        assert list(found) == tails
        assert {k: v for k, v in found.items() if v != (0, _lib.NO_MISMATCH)} == {}, which
    # and B's own records, as the run left them, are consistent chains too
    _run_b(gm, g.b)
    assert set(gm.module.check_chains().values()) == {(0, _lib.NO_MISMATCH)}


# ---------------------------------------------------------------- a producer's wrong convolution
@pytest.mark.parametrize("which", ["resnet18", "resnet50", "mobilenet_v2", "pad24"])
def test_wrong_convolution_with_a_consistent_tail_is_the_conv_alone(device, graphs, which):
    g = graphs(which)
    gm = g.gm
    chains = g.chains()
    node, recs = chains[len(chains) // 2]
    conv, rq = recs[0], recs[2]
    old = g.records
    # an element whose value passes through the tail: its last record is at neither end of its range
    last = old[recs[-1]].reshape(-1)
    inner = np.flatnonzero((last > last.min()) & (last < last.max()))
    flat = int(inner[len(inner) // 2])
    # the smallest power of two that moves the requantized value, by the oracle
    for k in range(31):
        new = {conv: _bump(old[conv], flat, 1 << k)}
        for r in recs[1:]:
            new[r] = g.eval(r, {**old, **new})
        if new[rq].reshape(-1)[flat] != old[rq].reshape(-1)[flat]:
            break
    else:
        pytest.fail("no amount changes the requantized value")
    changed = [r for r in recs if not np.array_equal(new[r], old[r])]
    assert conv in changed and rq in changed and len(changed) >= 3
    assert all(int((new[r] != old[r]).sum()) == 1 for r in changed)
    for blob in g.rewritten(new):
        _run_b(gm, g.b)
        rep = gm.replay_trace(blob)
        assert not rep.ok
        _consistent(rep)
        assert set(changed) <= {m.name for m in rep.mismatches}
        assert node in [n.node for n in rep.nodes]
        mine = [o for o in rep.ops if o.node == node]
        assert _brief(mine) == [(conv, "node", 1, flat)], mine
        assert mine[0].op == g.ops[conv] and mine[0].place == 0
        assert mine[0].first_index == tuple(int(i) for i in np.unravel_index(flat, old[conv].shape))
        assert next(n for n in rep.nodes if n.node == node).ops == mine
        # other faulty ops: only in nodes that read one of the changed records
        readers = {g.node_of[o.name] for o in gm.plan.ops if set(o.inputs) & set(changed)} - {node}
        assert all(o.node in readers for o in rep.ops if o.node != node), rep.ops
        # without the chain check the node is all one can name
        _run_b(gm, g.b)
        coarse = gm.replay_trace(blob, ops=False)
        assert coarse.ops == [] and [n.node for n in coarse.nodes] == [n.node for n in rep.nodes]


# ---------------------------------------------------------------- tail faults
@pytest.mark.parametrize("which", ["resnet18", "pad24"])
def test_a_bias_add_fault_that_the_requantize_absorbs(device, graphs, which):
    g = graphs(which)
    gm = g.gm
    chains = g.chains(3)
    node, recs = chains[len(chains) // 2]
    bias_add, rq = recs[1], recs[2]
    old = g.records
    flat = old[bias_add].size * 2 // 3
    while True:
        new = {bias_add: _bump(old[bias_add], flat)}
        if np.array_equal(g.eval(rq, {**old, **new}), old[rq]):   # by the oracle, the requantized value stays
            break
        flat += 1
    for blob in g.rewritten(new):
        _run_b(gm, g.b)
        rep = gm.replay_trace(blob)
        assert not rep.ok
        _consistent(rep)
        assert _brief(rep.ops) == [(bias_add, "input", 1, flat)], rep.ops
        assert rep.ops[0].node == node and rep.ops[0].place == 1 and rep.ops[0].op == "nn.bias_add"
        assert [m.name for m in rep.mismatches] == [bias_add] and [n.node for n in rep.nodes] == [node]


@pytest.mark.parametrize("which", ["resnet18", "pad24"])
def test_a_requantize_fault_below_the_clip(device, graphs, which):
    g = graphs(which)
    gm = g.gm
    old = g.records
    # a conv -> bias_add -> requantize -> clip block with a requantized value below the clip's lower
    # bound (and above the dtype's): moved down by one it is still clipped to the same value
    for node, recs in g.chains(4):
        if len(recs) != 4 or g.ops[recs[3]] not in ("clip", "nn.relu"):
            continue
        rq, clip = recs[2], recs[3]
        lo = int(old[clip].min())
        cand = np.flatnonzero((old[rq].reshape(-1) < lo) & (old[rq].reshape(-1) > np.iinfo(old[rq].dtype).min))
        if len(cand):
            break
    else:
        pytest.fail("no requantized value below a clip's lower bound")
    flat = int(cand[len(cand) // 2])
    new = {rq: old[rq].copy()}
    new[rq].reshape(-1)[flat] -= 1
    assert np.array_equal(g.eval(clip, {**old, **new}), old[clip])
    for blob in g.rewritten(new):
        _run_b(gm, g.b)
        rep = gm.replay_trace(blob)
        assert not rep.ok
        _consistent(rep)
        assert _brief(rep.ops) == [(rq, "input", 1, flat)], rep.ops
        assert rep.ops[0].node == node and rep.ops[0].place == 2 and rep.ops[0].op == "qnn.requantize"
        assert [m.name for m in rep.mismatches] == [rq]


# ---------------------------------------------------------------- two faults in one chain
@pytest.mark.parametrize("which", ["resnet50", "pad24"])
def test_two_faults_in_one_chain(device, graphs, which):
    g = graphs(which)
    gm = g.gm
    chains = [c for c in g.chains(4) if g.ops[c[1][-1]] in ("clip", "nn.relu")]
    node, recs = chains[len(chains) // 2]
    conv, bias_add, rq, clip = recs[0], recs[1], recs[2], recs[-1]
    old = g.records
    flat = old[conv].size // 3
    while True:
        # the conv moved by one, the bias_add consistent with it, the requantize unchanged by the oracle
        new = {conv: _bump(old[conv], flat)}
        new[bias_add] = g.eval(bias_add, {**old, **new})
        if np.array_equal(g.eval(rq, {**old, **new}), old[rq]):
            break
        flat += 1
    assert int((new[bias_add] != old[bias_add]).sum()) == 1
    at = old[clip].size - 2                                     # and the clip record, somewhere else
    new[clip] = _bump(old[clip], at)
    for blob in g.rewritten(new):
        _run_b(gm, g.b)
        rep = gm.replay_trace(blob)
        assert not rep.ok
        _consistent(rep)
        mine = [o for o in rep.ops if o.node == node]
        assert _brief(mine) == [(conv, "node", 1, flat), (clip, "input", 1, at)], mine
        assert {conv, bias_add, clip} <= {m.name for m in rep.mismatches}
        assert rq not in {m.name for m in rep.mismatches}
        assert next(n for n in rep.nodes if n.node == node).first == conv


# ---------------------------------------------------------------- ops=False, trace job
def test_without_ops_the_report_is_the_node_replay(device, graphs):
    g = graphs("pad24")
    gm = g.gm
    node, recs = g.chains(4)[0]
    blob = g.rewritten({recs[1]: _bump(g.records[recs[1]], 5, 1 << 20)})[1]
    _run_b(gm, g.b)
    fine = gm.replay_trace(blob)
    _run_b(gm, g.b)
    coarse = gm.replay_trace(blob, ops=False)
    assert coarse.ops == [] and "chain_ms" not in coarse.stats and "chain_ms" in fine.stats
    assert not coarse.ok and not fine.ok and fine.ops
    assert [(m.name, m.count, m.flat_index, m.node) for m in coarse.mismatches] == \
        [(m.name, m.count, m.flat_index, m.node) for m in fine.mismatches]
    assert [(n.node, n.kind, n.records, n.first) for n in coarse.nodes] == \
        [(n.node, n.kind, n.records, n.first) for n in fine.nodes]
    assert all(n.ops == [] for n in coarse.nodes) and coarse.first.name == fine.first.name
    assert set(fine.stats) - set(coarse.stats) == {"chain_ms"}
    for blob in g.files:
        _run_b(gm, g.b)
        rep = gm.replay_trace(blob, ops=False)
        assert rep.ok and rep.ops == [] and "chain_ms" not in rep.stats


@pytest.mark.parametrize("packed", [False, True])
def test_trace_job_check_replay_lists_ops(device, tmp_path, packed, capsys):
    d = str(tmp_path / "job")
    argv = ["--model", "lenet5", "--samples", "4", "--chunk", "2", "--out-dir", d]
    assert trace_job.main(argv + (["--packed"] if packed else [])) == 0
    capsys.readouterr()
    assert trace_job.main(argv + ["--check", "--replay"]) == 0
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert [r["chunk"] for r in lines] == [0, 1] and all(r["ok"] and r["ops"] == [] for r in lines)
    assert all(r["chain_ms"] >= 0 for r in lines)
    # one bit of chunk 1 changed: the last int32 record, the bias_add of the last dense block
    path = trace_job.chunk_file(d, 0, 1)
    plain = bytes(tf.unpack_trace(path)) if packed else open(path, "rb").read()
    trace = tf.read_trace(plain)
    name = [k for k in trace.records if trace.records[k].dtype == np.int32][-1]
    ct = tf.check_trace(plain, [(k, v.shape, str(v.dtype)) for k, v in trace.records.items()])
    e = next(e for e in ct.entries if e.name == name)
    blob = bytearray(plain)
    blob[ct.records_off + e.raw_off + 5 * 4] ^= 0x01             # element 5, its lowest bit
    src = str(tmp_path / "mod.tkt")
    open(src, "wb").write(tf.pack_trace(bytes(blob)) if packed else bytes(blob))
    shutil.copyfile(src, path)
    assert trace_job.main(argv + ["--check", "--replay"]) == 1
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert [r["ok"] for r in lines] == [True, False] and lines[0]["ops"] == []
    ops = lines[1]["ops"]
    assert len(ops) == 1 and ops[0]["name"] == name and ops[0]["op"] == "nn.bias_add"
    assert ops[0]["basis"] == "input" and ops[0]["place"] == 1 and ops[0]["count"] == 1
    assert ops[0]["first_index"] == list(np.unravel_index(5, trace.records[name].shape))
    assert ops[0]["node"] == lines[1]["nodes"][0]["node"]
