"""The chain check of a replay against the route there was before it, and replay_trace with and
without op granularity.

A ResNet-50 chunk of 64 samples is written once by the trace job, packed.  Then three interleaved
rounds, every run a fresh process, of

  chain        the chunk's records loaded into the module's buffers (load_trace), then
               tk_module_check_chains, HIP-event timed: the first call (which lays out and uploads
               the chain table) and the calls after it apart;
  parent       the same loaded records checked the way the entry points before the chain check allow:
               every tail op of every fused node by its stand-alone kernel (tk_bias_add,
               tk_requantize, tk_qnn_add, tk_clip) into scratch, then one tk_compare_device_batch
               of scratch against the records, HIP-event timed as one region;
  replay       GraphModule.replay_trace of the file, with its ``stats`` (chain_ms broken out);
  replay_node  the same with ops=False.

Before either route checks, the same few elements of four tail records are changed on the device,
so that the verdicts compared between the routes are not all "equal" (a record that reads a changed
one may differ with it, on both routes alike).  The chain check's rate is
given against a streaming read of the bytes it reads (every record of every fused chain and the
residual operands, once) at the 6.3 TB/s of HBM3E on the MI355X.

    python tools/bench_trace_replay_ops.py --out profiles/trace_replay_ops_resnet50.json [--dir SCRATCH]

The scratch directory (default: a fresh temporary one) holds about 4 GB while the tool runs and is
removed afterwards."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_trace_replay import _module, _spread, _timed, child_write  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
REPS = 5
BLOCKS = ("conv_block", "dense_block", "add_block")


def _loaded(args):
    """A module (no find step: the checks do not depend on the kernels chosen) whose buffers hold
    the chunk's records, with a few planted differences; the fused nodes; the bytes a check of
    their chains reads."""
    import torch
    proto, build_module = _module(args.model, args.chunk, tune=False)
    gm = build_module(args.chunk)
    gm.load_trace(args.packed)
    mod = gm.module
    nodes = [i for i, k in enumerate(mod.node_kinds) if k in BLOCKS and len(mod.node_records[i]) > 1]
    tails = [r for i in nodes for r in mod.node_records[i][1:]]
    for k, name in enumerate(tails[len(tails) // 5::len(tails) // 4][:4]):
        flat = mod.buffers[name].reshape(-1)
        at = [7, flat.numel() // 2 + k, flat.numel() - 1][:k + 1]
        flat[at] += 1
    torch.cuda.synchronize()
    nbytes = 0
    for i in nodes:
        n = mod._nodes[i]
        nbytes += sum(mod.buffers[r].numel() * mod.buffers[r].element_size() for r in mod.node_records[i])
        if mod.node_kinds[i] != "add_block" and n.attrs.block.has_add:
            nbytes += mod.buffers[mod.node_records[i][2]].numel()
    return gm, nodes, tails, nbytes


def child_chain(args) -> dict:
    gm, nodes, tails, nbytes = _loaded(args)
    try:
        mod = gm.module
        found = {}
        first = _timed(lambda: found.update(mod.check_chains()))
        ms = [_timed(mod.check_chains) for _ in range(REPS)]
        med = statistics.median(ms)
        assert list(found) == tails
        return {"route": "chain", "ops": len(tails), "nodes": len(nodes), "read_bytes": nbytes, "first_ms": first,
                "ms": ms, "median_ms": med, "GBps": nbytes / med / 1e6,
                "of_streaming_read": nbytes / (med * 1e-3) / HBM_BYTES_PER_S,
                "verdicts": {k: list(v) for k, v in found.items() if v[0]}}
    finally:
        gm.close()


def child_parent(args) -> dict:
    import torch
    from tachikoma_amd import _lib
    gm, nodes, tails, nbytes = _loaded(args)
    try:
        mod = gm.module
        lib = mod.lib
        s = ctypes.c_void_p(_lib.stream_handle(None))
        scratch = {r: torch.empty_like(mod.buffers[r]) for r in tails}
        sref = {r: _lib.TensorRef.from_torch(t) for r, t in scratch.items()}
        calls = []  # (function, arguments) of every stand-alone launch
        for i in nodes:
            n, recs = mod._nodes[i], mod.node_records[i]
            ref = [mod._ref(r).ptr for r in recs]
            if mod.node_kinds[i] == "add_block":
                ab = n.attrs.add_block
                calls.append((lib.tk_clip, (ref[0], sref[recs[1]].ptr, ab.clip_min, ab.clip_max, s)))
                continue
            ba = n.attrs.block
            calls.append((lib.tk_bias_add, (ref[0], n.inputs[2], sref[recs[1]].ptr, 1, s)))
            calls.append((lib.tk_requantize, (ref[1], sref[recs[2]].ptr, ctypes.byref(ba.requantize), s)))
            last = 2
            if ba.has_add:
                lhs, rhs = (n.inputs[3], ref[2]) if ba.block_is_rhs else (ref[2], n.inputs[3])
                calls.append((lib.tk_qnn_add, (lhs, rhs, sref[recs[3]].ptr, ctypes.byref(ba.add), s)))
                last = 3
            if ba.has_clip:
                calls.append((lib.tk_clip, (ref[last], sref[recs[last + 1]].ptr, ba.clip_min, ba.clip_max, s)))
        k = len(tails)
        exp = (ctypes.c_void_p * k)(*[scratch[r].data_ptr() for r in tails])
        got = (ctypes.c_void_p * k)(*[mod.buffers[r].data_ptr() for r in tails])
        cnt = (ctypes.c_int64 * k)(*[mod.buffers[r].numel() for r in tails])
        es = (ctypes.c_int32 * k)(*[mod.buffers[r].element_size() for r in tails])
        report = (_lib.tk_wire_mismatch * k)()

        def route():
            for fn, a in calls:
                _lib.check(fn(*a), "stand-alone op")
            _lib.check(lib.tk_compare_device_batch(exp, got, cnt, es, k, report, s), "tk_compare_device_batch")

        first = _timed(route)
        ms = [_timed(route) for _ in range(REPS)]
        med = statistics.median(ms)
        moved = sum(scratch[r].numel() * scratch[r].element_size() for r in tails)
        return {"route": "parent", "ops": k, "launches": len(calls) + 2, "first_ms": first, "ms": ms, "median_ms": med,
                "moved_bytes": nbytes + 2 * moved,  # inputs read, scratch written, scratch and records compared
                "verdicts": {r: [int(x.mismatches), int(x.first)] for r, x in zip(tails, report) if x.mismatches}}
    finally:
        gm.close()


def _end_to_end(args, ops: bool) -> dict:
    import torch
    proto, build_module = _module(args.model, args.chunk)
    gm = build_module(args.chunk)
    try:
        gm.trace_verifier()                # the staging and the device buffer, sized once
        torch.cuda.synchronize()
        out = []
        for _ in range(2):                 # the second call has everything warm
            t0 = time.perf_counter()
            rep = gm.replay_trace(args.packed, ops=ops)
            out.append({"total_ms": (time.perf_counter() - t0) * 1e3, "ok": bool(rep.ok), "n_ops": len(rep.ops),
                        "stats": dict(rep.stats)})
        return {"route": "replay" if ops else "replay_node", **out[0], "second": out[1]}
    finally:
        gm.close()


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model", default="resnet50")
    p.add_argument("--chunk", type=int, default=64)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--dir", default=None)
    p.add_argument("--out", default=None)
    p.add_argument("--child", choices=["write", "chain", "parent", "replay", "replay_node"], default=None)
    p.add_argument("--packed", default=None)
    args = p.parse_args()
    if args.child:
        fn = {"write": child_write, "chain": child_chain, "parent": child_parent,
              "replay": lambda a: _end_to_end(a, True), "replay_node": lambda a: _end_to_end(a, False)}[args.child]
        print("RESULT " + json.dumps(fn(args)), flush=True)
        return 0
    made = args.dir is None
    args.dir = tempfile.mkdtemp(prefix="tk_replay_ops_") if made else args.dir
    os.makedirs(args.dir, exist_ok=True)

    def run(child, *extra):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--model", args.model, "--chunk",
               str(args.chunk), "--dir", args.dir, *extra]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True)
        line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
        print(f"[bench_trace_replay_ops] {child}: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        return json.loads(line[7:])

    try:
        file = run("write")
        rounds = []
        for _ in range(args.rounds):
            rounds.append({k: run(k, "--packed", file["file"]) for k in ("chain", "parent", "replay", "replay_node")})
    finally:
        if made:
            shutil.rmtree(args.dir, ignore_errors=True)
    chain, parent = [r["chain"] for r in rounds], [r["parent"] for r in rounds]
    rep, node = [r["replay"] for r in rounds], [r["replay_node"] for r in rounds]
    out = {"model": args.model, "chunk": args.chunk, "file": dict(file, file=os.path.relpath(file["file"], args.dir)),
           "rounds": rounds,
           "tail_ops": chain[0]["ops"], "fused_nodes": chain[0]["nodes"], "chain_read_bytes": chain[0]["read_bytes"],
           "parent_launches": parent[0]["launches"], "parent_moved_bytes": parent[0]["moved_bytes"],
           "chain_ms": _spread([c["median_ms"] for c in chain]),
           "chain_first_call_ms": _spread([c["first_ms"] for c in chain]),
           "chain_GBps": _spread([c["GBps"] for c in chain]),
           "chain_of_streaming_read": _spread([c["of_streaming_read"] for c in chain]),
           "parent_ms": _spread([c["median_ms"] for c in parent]),
           "replay_total_ms": _spread([v["total_ms"] for v in rep]),
           "replay_node_total_ms": _spread([v["total_ms"] for v in node]),
           "replay_second_total_ms": _spread([v["second"]["total_ms"] for v in rep]),
           "replay_node_second_total_ms": _spread([v["second"]["total_ms"] for v in node]),
           "replay_chain_ms": _spread([v["second"]["stats"]["chain_ms"] for v in rep]),
           **{f"replay_{k}": _spread([v["second"]["stats"][k] for v in rep]) for k in ("store_ms", "shadow_ms", "replay_ms",
                                                                                       "compare_ms", "run_ms")},
           **{f"replay_node_{k}": _spread([v["second"]["stats"][k] for v in node]) for k in ("store_ms", "shadow_ms",
                                                                                             "replay_ms", "compare_ms",
                                                                                             "run_ms")},
           "planted_verdicts": chain[0]["verdicts"],
           # (at least the four planted records; a record that reads a planted one may differ too)
           "verdicts_equal": all(r["chain"]["verdicts"] == r["parent"]["verdicts"] and len(r["chain"]["verdicts"]) >= 4
                                 for r in rounds),
           "all_ok": all(v["ok"] and v["second"]["ok"] and v["n_ops"] == 0 for v in rep + node)}
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in out.items() if k != "rounds"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
