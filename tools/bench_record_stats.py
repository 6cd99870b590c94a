"""The statistics kernel on a ResNet-50 chunk, against a streaming read and against the route there
was before it.

Interleaved rounds, every run a fresh process, of

  module      a 64-sample ResNet-50 module after one run: one tk_stats_plan_run over all its records
              (StatsAccumulator.add), HIP-event timed, the first call and the calls after it apart;
              the bytes it reads, its fraction of a streaming read at the 6.3 TB/s of HBM3E on the
              MI355X, and the bytes its workgroups flush (an upper bound from the result: every
              workgroup of a record flushing every bin the record's histograms use);
  synthetic   the same launch over one synthetic record of that many bytes, int8 and int32, once all
              zeros and once uniform over the dtype's range: the two ends of the histogram
              contention;
  stats_only  the per-chunk wall time of the trace job's --stats-only route (run, one statistics
              launch, nothing leaves the device), over several chunks after a warm-up chunk;
  parent      the same numbers the way the entry points before the kernel allow: a default traced
              step (every record copied to the host image) and trace_format.record_stats over the
              image's records on the host, timed apart.

    python tools/bench_record_stats.py --out profiles/record_stats_resnet50.json"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_trace_replay import _module, _spread, _timed  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
REPS = 5


def _rate(nbytes: int, ms: float) -> dict:
    return {"GBps": nbytes / ms / 1e6, "of_streaming_read": nbytes / (ms * 1e-3) / HBM_BYTES_PER_S}


def child_module(args) -> dict:
    import torch
    from tachikoma_amd import _lib
    proto, build_module = _module(args.model, args.chunk, tune=False)
    gm = build_module(args.chunk)
    try:
        gm.set_input(proto.input_name, proto.sample_inputs(0, args.chunk))
        gm.run()
        acc = gm.stats_accumulator()
        torch.cuda.synchronize()
        first = _timed(acc.add)
        ms = [_timed(acc.add) for _ in range(REPS)]
        acc.reset()
        acc.add()
        res = acc.result()
        span = _lib.load().tk_record_stats_span()
        bufs = gm.module.buffers
        nbytes = sum(bufs[n].numel() * bufs[n].element_size() for n in acc.names)
        groups = {n: -(-bufs[n].numel() // span) for n in acc.names}
        words = {n: 4 + int((s.bits != 0).sum()) + (0 if s.values is None else int((s.values != 0).sum()))
                 for n, s in res.items()}
        flushed = sum(8 * groups[n] * words[n] for n in acc.names)
        worst = sum(8 * groups[n] * (4 + 33 + (0 if res[n].values is None else 256)) for n in acc.names)
        med = statistics.median(ms)
        return {"route": "module", "records": len(acc.names), "skipped": len(acc.skipped), "read_bytes": nbytes,
                "workgroups": sum(groups.values()), "flushed_bytes_bound": flushed, "flushed_bytes_worst_case": worst,
                "flushed_over_read": flushed / nbytes, "first_ms": first, "ms": ms, "median_ms": med, **_rate(nbytes, med),
                "elements": sum(s.count for s in res.values())}
    finally:
        gm.close()


def child_synthetic(args) -> dict:
    import torch
    from tachikoma_amd import _lib
    from tachikoma_amd import trace_format as tf
    lib = _lib.load()
    torch.cuda.set_device(0)
    nbytes = int(args.bytes) // 16 * 16
    raw = torch.zeros(nbytes, dtype=torch.int8, device="cuda")
    stats = torch.zeros(tf.STATS_DTYPE.itemsize // 8, dtype=torch.int64, device="cuda")
    s = ctypes.c_void_p(_lib.stream_handle(None))
    out = {"route": "synthetic", "read_bytes": nbytes}
    for fill in ("zeros", "uniform"):
        if fill == "uniform":
            step = 1 << 28
            for at in range(0, nbytes, step):
                n = min(step, nbytes - at)
                raw[at:at + n] = torch.randint(-128, 128, (n,), dtype=torch.int8, device="cuda")
        for kind, name, es in ((1, "int8", 1), (0, "int32", 4)):
            plan = ctypes.c_void_p()
            _lib.check(lib.tk_stats_plan_create((ctypes.c_void_p * 1)(raw.data_ptr()), (ctypes.c_int64 * 1)(nbytes // es),
                                                (ctypes.c_int32 * 1)(kind), 1, ctypes.byref(plan)), "tk_stats_plan_create")
            _lib.check(lib.tk_record_stats_reset(ctypes.c_void_p(stats.data_ptr()), 1, s), "tk_record_stats_reset")
            run = lambda: _lib.check(lib.tk_stats_plan_run(plan, ctypes.c_void_p(stats.data_ptr()), s), "run")  # noqa: E731
            first = _timed(run)
            ms = [_timed(run) for _ in range(REPS)]
            lib.tk_stats_plan_destroy(plan)
            row = stats.cpu().numpy().view(tf.STATS_DTYPE)[0]
            assert int(row["count"]) == (REPS + 1) * (nbytes // es)
            med = statistics.median(ms)
            out[f"{name}_{fill}"] = {"first_ms": first, "ms": ms, "median_ms": med, **_rate(nbytes, med)}
    return out


def child_stats_only(args) -> dict:
    import torch
    from tachikoma_amd import trace_job
    proto, build_module = _module(args.model, args.chunk)
    tracer = trace_job.GraphModuleTracer(build_module, proto.sample_inputs, model=proto.name,
                                         input_name=proto.input_name)
    try:
        tracer.stats_only(0, args.chunk)      # warm-up: the module, its graph, the plan
        torch.cuda.synchronize()
        acc = tracer.accumulator(args.chunk)
        acc.reset()
        t0 = time.perf_counter()
        for c in range(args.chunks):
            tracer.stats_only(c * args.chunk, args.chunk)
        res = acc.result()
        ms = (time.perf_counter() - t0) * 1e3
        gm = tracer.modules[args.chunk][0]
        stream = torch.cuda.current_stream(gm.module.device)
        # the device's share of a chunk: the compute-only run and the statistics launch, inputs in place
        dev = [_timed(lambda: (gm.module.run(stream), acc.add(stream))) for _ in range(REPS)]
        return {"route": "stats_only", "chunks": args.chunks, "total_ms": ms, "per_chunk_ms": ms / args.chunks,
                "device_ms": dev, "device_median_ms": statistics.median(dev),
                "elements": sum(s.count for s in res.values())}
    finally:
        tracer.close()


def child_parent(args) -> dict:
    import torch
    from tachikoma_amd import trace_format as tf
    proto, build_module = _module(args.model, args.chunk)
    gm = build_module(args.chunk)
    try:
        cap = gm.trace_capture()
        gm.set_input(proto.input_name, proto.sample_inputs(0, args.chunk))
        gm.run(trace=True)                    # warm-up
        cap.synchronize()
        torch.cuda.synchronize()
        steps = []
        for c in range(args.chunks):
            t0 = time.perf_counter()      # as stats_only: the chunk's inputs are made and set inside
            gm.set_input(proto.input_name, proto.sample_inputs(c * args.chunk, args.chunk))
            gm.run(trace=True)
            cap.synchronize()
            torch.cuda.synchronize()
            steps.append((time.perf_counter() - t0) * 1e3)
        records = tf.read_trace(cap.bytes()).records
        t0 = time.perf_counter()
        res = {}
        for k, v in records.items():
            if str(v.dtype) in tf.STATS_KIND:
                res[k] = tf.record_stats(v, k)
                if len(res) % 16 == 0:
                    print(f"[bench_record_stats] parent: {len(res)} records reduced", file=sys.stderr, flush=True)
        host_ms = (time.perf_counter() - t0) * 1e3
        step = statistics.median(steps)
        return {"route": "parent", "traced_step_ms": steps, "traced_step_median_ms": step, "host_reduce_ms": host_ms,
                "per_chunk_ms": step + host_ms, "elements": sum(s.count for s in res.values())}
    finally:
        gm.close()


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model", default="resnet50")
    p.add_argument("--chunk", type=int, default=64)
    p.add_argument("--chunks", type=int, default=4, help="chunks timed per stats_only / parent run")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--parent-rounds", type=int, default=1,
                   help="rounds that also take the parent route (its host reduction takes minutes)")
    p.add_argument("--out", default=None)
    p.add_argument("--child", choices=["module", "synthetic", "stats_only", "parent"], default=None)
    p.add_argument("--bytes", default=None)
    args = p.parse_args()
    if args.child:
        fn = {"module": child_module, "synthetic": child_synthetic, "stats_only": child_stats_only,
              "parent": child_parent}[args.child]
        print("RESULT " + json.dumps(fn(args)), flush=True)
        return 0

    def run(child, *extra):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--model", args.model, "--chunk",
               str(args.chunk), "--chunks", str(args.chunks), *extra]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True)
        line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
        print(f"[bench_record_stats] {child}: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        return json.loads(line[7:])

    rounds = []
    for k in range(args.rounds):
        row = {"module": run("module")}
        row["synthetic"] = run("synthetic", "--bytes", str(row["module"]["read_bytes"]))
        row["stats_only"] = run("stats_only")
        if k < args.parent_rounds:
            row["parent"] = run("parent")
        rounds.append(row)
    mod = [r["module"] for r in rounds]
    syn = [r["synthetic"] for r in rounds]
    only = [r["stats_only"] for r in rounds]
    par = [r["parent"] for r in rounds if "parent" in r]
    out = {"model": args.model, "chunk": args.chunk, "rounds": rounds,
           "records": mod[0]["records"], "skipped": mod[0]["skipped"], "read_bytes": mod[0]["read_bytes"],
           "workgroups": mod[0]["workgroups"], "flushed_bytes_bound": mod[0]["flushed_bytes_bound"],
           "flushed_over_read": mod[0]["flushed_over_read"],
           "stats_ms": _spread([m["median_ms"] for m in mod]),
           "stats_first_call_ms": _spread([m["first_ms"] for m in mod]),
           "stats_GBps": _spread([m["GBps"] for m in mod]),
           "stats_of_streaming_read": _spread([m["of_streaming_read"] for m in mod]),
           **{f"synthetic_{k}_ms": _spread([s[k]["median_ms"] for s in syn])
              for k in ("int8_zeros", "int8_uniform", "int32_zeros", "int32_uniform")},
           **{f"synthetic_{k}_of_streaming_read": _spread([s[k]["of_streaming_read"] for s in syn])
              for k in ("int8_zeros", "int8_uniform", "int32_zeros", "int32_uniform")},
           "stats_only_per_chunk_ms": _spread([o["per_chunk_ms"] for o in only]),
           "stats_only_device_ms": _spread([o["device_median_ms"] for o in only]),
           "parent_per_chunk_ms": _spread([v["per_chunk_ms"] for v in par]) if par else None,
           "parent_traced_step_ms": _spread([v["traced_step_median_ms"] for v in par]) if par else None,
           "parent_host_reduce_ms": _spread([v["host_reduce_ms"] for v in par]) if par else None,
           "counter_run": False}
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in out.items() if k != "rounds"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
