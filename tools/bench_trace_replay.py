"""Replaying a packed trace chunk op by op: the batched shadow rebuild against the loop it replaces,
and replay_trace against verify_trace.

A ResNet-50 chunk of 64 samples is written once by the trace job, packed.  Then three interleaved
rounds, every run a fresh process, of

  single  every record-sourced shadow of the module rebuilt by a loop of tk_conv2d_make_shadow (one
          launch per tensor: what there was before the batched call), HIP-event timed;
  batch   the same shadows by one tk_conv2d_make_shadow_batch call, HIP-event timed: the first call
          (which lays out and uploads the item table) and the calls after it apart;
  verify  GraphModule.verify_trace of the packed file, with its ``stats``;
  replay  GraphModule.replay_trace of the same file, with its ``stats`` (store_ms, shadow_ms,
          replay_ms broken out).

Both shadow routes run on the records of one run of the module and are compared byte for byte in
the batch child.  The rebuild's rate is given as a fraction of a streaming copy of the same bytes:
one byte read and one written per shadow element, against the 6.3 TB/s of HBM3E on the MI355X.

    python tools/bench_trace_replay.py --out profiles/trace_replay_resnet50.json [--dir SCRATCH]

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

HBM_BYTES_PER_S = 6.3e12
REPS = 5


def _module(model: str, n: int, tune=True):
    import torch
    from tachikoma_amd import relay, zoo
    from tachikoma_amd.contrib import graph_executor
    torch.cuda.set_device(0)
    model_fn = zoo.MODELS[model]
    proto = model_fn(batch=1)

    def build_module(k):
        mdl = model_fn(batch=k)
        lib = relay.build(mdl.mod, target="mi355x", params=mdl.params)
        return graph_executor.GraphModule(lib["default"](0, tune=tune))

    return proto, build_module


def child_write(args) -> dict:
    from tachikoma_amd import trace_job
    proto, build_module = _module(args.model, args.chunk)
    d = os.path.join(args.dir, "packed")
    tracer = trace_job.GraphModuleTracer(build_module, proto.sample_inputs, model=proto.name,
                                         input_name=proto.input_name, packed=True)
    try:
        entries = trace_job.run(tracer, args.chunk, args.chunk, d, resume=False, packed=True)
    finally:
        tracer.close()
    path = os.path.join(d, entries[0].file)
    return {"file": path, "bytes": os.path.getsize(path), "digest": entries[0].digest}


def _shadow_setup(args):
    """A module that has run once on the chunk's samples (no find step: the shadows do not depend
    on the kernels chosen), and its record-sourced shadows."""
    import torch
    proto, build_module = _module(args.model, args.chunk, tune=False)
    gm = build_module(args.chunk)
    gm.set_input(proto.input_name, proto.sample_inputs(0, args.chunk))
    gm.run()
    torch.cuda.synchronize()
    mod = gm.module
    names = mod.replay_plan()[1]
    refs = [mod.shadow_sources[s][0] for s in names]
    bufs = [mod.shadow_sources[s][1] for s in names]
    nbytes = [int(mod.lib.tk_conv2d_shadow_bytes(r.ptr)) for r in refs]
    return gm, names, refs, bufs, nbytes


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _rates(ms: float, total: int) -> dict:
    moved = 2 * total
    return {"GBps": moved / ms / 1e6, "of_streaming_copy": moved / (ms * 1e-3) / HBM_BYTES_PER_S}


def child_single(args) -> dict:
    from tachikoma_amd import _lib
    gm, names, refs, bufs, nbytes = _shadow_setup(args)
    try:
        lib = gm.module.lib
        s = ctypes.c_void_p(_lib.stream_handle(None))

        def loop():
            for r, b in zip(refs, bufs):
                _lib.check(lib.tk_conv2d_make_shadow(r.ptr, ctypes.c_void_p(b.data_ptr()), s), "tk_conv2d_make_shadow")

        first = _timed(loop)
        ms = [_timed(loop) for _ in range(REPS)]
        med = statistics.median(ms)
        return {"route": "single", "shadows": len(names), "shadow_bytes": sum(nbytes), "first_ms": first, "ms": ms,
                "median_ms": med, **_rates(med, sum(nbytes))}
    finally:
        gm.close()


def child_batch(args) -> dict:
    import torch
    from tachikoma_amd import _lib
    gm, names, refs, bufs, nbytes = _shadow_setup(args)
    try:
        mod = gm.module
        lib = mod.lib
        s = ctypes.c_void_p(_lib.stream_handle(None))
        for r, b in zip(refs, bufs):  # the reference bytes, by the single-tensor kernel
            _lib.check(lib.tk_conv2d_make_shadow(r.ptr, ctypes.c_void_p(b.data_ptr()), s), "tk_conv2d_make_shadow")
        want = [b[:n].clone() for b, n in zip(bufs, nbytes)]
        for b in bufs:
            b.fill_(0xA5)
        first = _timed(lambda: mod.rebuild_shadows(names))
        equal = all(bool(torch.equal(b[:n], w)) for b, n, w in zip(bufs, nbytes, want))
        ms = [_timed(lambda: mod.rebuild_shadows(names)) for _ in range(REPS)]
        med = statistics.median(ms)
        return {"route": "batch", "shadows": len(names), "shadow_bytes": sum(nbytes), "first_ms": first, "ms": ms,
                "median_ms": med, "equal": equal, **_rates(med, sum(nbytes))}
    finally:
        gm.close()


def _end_to_end(args, replay: bool) -> dict:
    import torch
    proto, build_module = _module(args.model, args.chunk)
    gm = build_module(args.chunk)
    try:
        gm.trace_verifier()                # the staging and the device buffer, sized once
        torch.cuda.synchronize()
        call = gm.replay_trace if replay else gm.verify_trace
        t0 = time.perf_counter()
        rep = call(args.packed)
        total = (time.perf_counter() - t0) * 1e3
        t1 = time.perf_counter()
        rep2 = call(args.packed)           # the same file again, everything warm
        total2 = (time.perf_counter() - t1) * 1e3
        return {"route": "replay" if replay else "verify", "total_ms": total, "ok": bool(rep.ok),
                "n_records": rep.n_records, "stats": dict(rep.stats),
                "second": {"total_ms": total2, "ok": bool(rep2.ok), "stats": dict(rep2.stats)}}
    finally:
        gm.close()


def _spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model", default="resnet50")
    p.add_argument("--chunk", type=int, default=64)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--dir", default=None)
    p.add_argument("--out", default=None)
    p.add_argument("--child", choices=["write", "single", "batch", "verify", "replay"], default=None)
    p.add_argument("--packed", default=None)
    args = p.parse_args()
    if args.child:
        fn = {"write": child_write, "single": child_single, "batch": child_batch,
              "verify": lambda a: _end_to_end(a, False), "replay": lambda a: _end_to_end(a, True)}[args.child]
        print("RESULT " + json.dumps(fn(args)), flush=True)
        return 0
    made = args.dir is None
    args.dir = tempfile.mkdtemp(prefix="tk_replay_") if made else args.dir
    os.makedirs(args.dir, exist_ok=True)

    def run(child, *extra):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--model", args.model, "--chunk",
               str(args.chunk), "--dir", args.dir, *extra]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True)
        line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
        print(f"[bench_trace_replay] {child}: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        return json.loads(line[7:])

    try:
        file = run("write")
        rounds = []
        for _ in range(args.rounds):
            rounds.append({k: run(k, "--packed", file["file"]) for k in ("single", "batch", "verify", "replay")})
    finally:
        if made:
            shutil.rmtree(args.dir, ignore_errors=True)
    single, batch = [r["single"] for r in rounds], [r["batch"] for r in rounds]
    ver, rep = [r["verify"] for r in rounds], [r["replay"] for r in rounds]
    out = {"model": args.model, "chunk": args.chunk, "file": dict(file, file=os.path.relpath(file["file"], args.dir)),
           "rounds": rounds,
           "shadows": batch[0]["shadows"], "shadow_bytes": batch[0]["shadow_bytes"],
           "single_ms": _spread([s["median_ms"] for s in single]),
           "batch_ms": _spread([b["median_ms"] for b in batch]),
           "batch_first_call_ms": _spread([b["first_ms"] for b in batch]),
           "single_of_streaming_copy": _spread([s["of_streaming_copy"] for s in single]),
           "batch_of_streaming_copy": _spread([b["of_streaming_copy"] for b in batch]),
           "batch_GBps": _spread([b["GBps"] for b in batch]),
           "verify_total_ms": _spread([v["total_ms"] for v in ver]),
           "replay_total_ms": _spread([v["total_ms"] for v in rep]),
           "verify_second_total_ms": _spread([v["second"]["total_ms"] for v in ver]),
           "replay_second_total_ms": _spread([v["second"]["total_ms"] for v in rep]),
           **{f"verify_{k}": _spread([v["stats"][k] for v in ver]) for k in ("read_ms", "check_ms", "upload_ms", "run_ms",
                                                                             "compare_ms")},
           **{f"replay_{k}": _spread([v["stats"][k] for v in rep]) for k in ("read_ms", "check_ms", "upload_ms", "run_ms",
                                                                             "store_ms", "shadow_ms", "replay_ms",
                                                                             "compare_ms")},
           "all_ok": all(r["batch"]["equal"] and r["verify"]["ok"] and r["replay"]["ok"] and r["verify"]["second"]["ok"]
                         and r["replay"]["second"]["ok"] for r in rounds)}
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in out.items() if k != "rounds"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
