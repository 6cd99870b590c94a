"""The schedule of a trace replay (GraphModule.replay_trace): pure host logic over the plain data
DeviceModule keeps while it emits nodes.  Imports nothing but the standard library.

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

from typing import Dict, Iterable, List, Sequence, Tuple


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
