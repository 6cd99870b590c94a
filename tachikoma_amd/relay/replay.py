"""The schedule of a trace replay (GraphModule.replay_trace) and the attribution of its findings to
ops (attribute_ops, at the end): pure host logic over the plain data DeviceModule keeps while it
emits nodes.  Imports nothing but the standard library.

``node_io[k]`` describes node k of the native module::

    {"kind": str,                 # for messages
     "records": [names],          # the trace records the node writes (empty: a helper node)
     "reads": [names],            # every buffer it reads: records, graph inputs, shadows, scratch
     "writes": [names],           # every buffer it writes: its records, shadows, scratch
     "shadows": {shadow: source}} # of the shadows among ``writes``: the tensor each is the shadow of

Params and what is derived from params alone (packed weights, weight sums, transposed weights)
are constants of a replay and are not listed.

The replay loads every record of a file into the module's buffers, rebuilds the shadows whose
source is a record, and runs the record-producing nodes in reverse topological order.  When node k
runs, every record it reads still holds what the file recorded: only outputs of later nodes have
been overwritten, and k reads none of them.  Node k then overwrites its own records (and the shadow
its epilogue writes) with what this engine computes from the recorded inputs; its consumers have
already run.

Helper nodes write no record: shadow nodes, the transposes of a layout conv, the contraction of a
BYOC composite.  Their outputs live in scratch that a later node reads, so a *unit* is one
record-producing node preceded, in forward order, by every helper it depends on through non-record
buffers, transitively; a helper two units need runs in both.  A shadow whose source is a record
or a graph input is rebuilt up front (one batched launch) and is no dependency; a shadow of a
non-record tensor is rebuilt by the helpers of the unit that reads it.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Tuple


class UnsupportedError(NotImplementedError):
    pass


def replay_units(node_io: Sequence[dict], inputs: Iterable[str] = ()) -> Tuple[List[List[int]], List[str]]:
    """(units in forward order, shadows to rebuild up front).  A unit is a list of node indices in
    forward order whose last is its record-producing node.  ``inputs``: the graph inputs (records
    of the file that no node writes)."""
    records = set(inputs)
    shadow_src: Dict[str, str] = {}
    for io in node_io:
        records.update(io.get("records", ()))
        for s, src in io.get("shadows", {}).items():
            shadow_src.setdefault(s, src)
    upfront = [s for s, src in shadow_src.items() if src in records]
    satisfied = records | set(upfront)

    def writer(b: str, before: int):
        """The last helper node before ``before`` that writes ``b``."""
        for j in range(before - 1, -1, -1):
            if b in node_io[j].get("writes", ()) and not node_io[j].get("records"):
                return j
        return None

    units = []
    for k, io in enumerate(node_io):
        if not io.get("records"):
            continue
        need, stack = set(), [k]
        while stack:
            i = stack.pop()
            for b in node_io[i].get("reads", ()):
                if b in satisfied:
                    continue
                j = writer(b, i)
                if j is None:
                    raise UnsupportedError(f"replay: node {i} ({node_io[i].get('kind', '?')}) reads {b!r}, which is "
                                           f"no record and which no helper node before it and no up-front shadow "
                                           f"rebuild produces")
                if j not in need:
                    need.add(j)
                    stack.append(j)
        units.append(sorted(need) + [k])
    return units, upfront


def replay_order(node_io: Sequence[dict], inputs: Iterable[str] = ()) -> Tuple[List[int], List[str]]:
    """(node order of a replay, shadows to rebuild up front): the units of ``replay_units`` in
    reverse order of their record node, each unit's nodes in forward order.  Raises
    UnsupportedError, naming the node, when a node reads a non-record buffer that no helper node
    before it and no up-front rebuild produces."""
    units, upfront = replay_units(node_io, inputs)
    return [i for u in reversed(units) for i in u], upfront


def attribute_ops(nodes: Sequence[Tuple[int, Sequence[str]]], mismatches: Mapping[str, Tuple[int, int]],
                  chain: Optional[Mapping[str, Tuple[int, int]]] = None) -> List[dict]:
    """One verdict per op from the two checks of a replay.

    ``nodes``: (node index, its records in chain order) of every record-producing node, in node
    order.  ``mismatches``: {record: (count, first flat index)} of the replay compare -- the record
    differs from what this engine computes from the recorded inputs of its *node*; records that are
    equal may be left out or carry a count of 0; names that are no node's record (graph inputs) are
    ignored.  ``chain``: {record: (count, first)} of the chain check -- the tail record is not the op
    of its own recorded *input*; it holds every tail record that was checked, equal ones with a
    count of 0.  None: no chain check was made.

    Returns the faulty ops in node order, then chain order, each as
    {"name", "node", "place" (index in the chain), "basis", "count", "first"}:

    - the head op of a node (place 0; the only op of an unfused node) is faulty when its record
      differs in the replay: basis "node";
    - a tail op the chain check covers is faulty when the chain check says so, whatever the replay
      says of its record: basis "input".  A producer's fault that the tail carries on consistently
      is therefore the producer's alone, and a second fault further down the chain is found;
    - where the chain check does not cover a node's tail, the node keeps node granularity: its
      first differing record stands for it, basis "node"."""
    out: List[dict] = []

    def bad(table, name):
        c = table.get(name)
        return c if c is not None and c[0] else None

    for node, records in nodes:
        records = list(records)
        if not records:
            continue
        tail = records[1:]
        covered = chain is not None and all(r in chain for r in tail)
        if covered:
            head = bad(mismatches, records[0])
            if head:
                out.append({"name": records[0], "node": node, "place": 0, "basis": "node", "count": head[0],
                            "first": head[1]})
            for k, r in enumerate(tail, 1):
                c = bad(chain, r)
                if c:
                    out.append({"name": r, "node": node, "place": k, "basis": "input", "count": c[0], "first": c[1]})
        else:
            for k, r in enumerate(records):
                c = bad(mismatches, r)
                if c:
                    out.append({"name": r, "node": node, "place": k, "basis": "node", "count": c[0], "first": c[1]})
                    break
    return out
