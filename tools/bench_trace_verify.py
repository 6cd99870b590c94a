"""Checking a packed trace chunk against the engine: the host route against verify_trace.

A ResNet-50 chunk of 64 samples is written once by the trace job, packed, together with an unpacked
dump of the same samples.  Then three interleaved rounds, every run a fresh process, of

  host    the route without a device decoder: trace_format.unpack_trace of the packed chunk, then a
          NumPy compare of its records section against the unpacked dump's;
  device  GraphModule.verify_trace of the same packed file (read into pinned staging, checked on
          the host, uploaded as it is, one compute-only run from the file's input, then the decode
          kernel's compare mode), with its ``stats`` split.  The module build, the find step and
          the verifier's buffers are set up before the clock starts, as a trace job has them.

Per route: median and min-max of the total, and for the device route of every part.  Next to them
the achieved rates: the upload in GB/s against a pinned H2D copy of the same bytes timed in the same
process (the probe), and the compare call's wire plus record bytes per second.

    python tools/bench_trace_verify.py --out profiles/trace_verify_resnet50.json [--dir SCRATCH]

With ``--bias`` the packed chunk is a version-3 file (the trace job's ``--packed --bias-coding``).
With ``--kernel-times`` the tool measures the decode kernels alone instead: the chunk is written
(``--bias`` or not), and one device run per ``--tree`` (default: this tree; a parent checkout with its
library built may be named beside it) is taken under ``rocprofv3 --kernel-trace --stats``, each a
profiler run of its own with that tree's copy of this tool as the program; reported are the rows of
``wire_decode_kernel`` from the profiler's kernel statistics (calls, total, average, min, max in ns;
a device run verifies twice, so compare mode has two calls) and the rate of wire plus record bytes
at the compare instantiation's average.

    python tools/bench_trace_verify.py --kernel-times --tree . PARENT [--bias] --out kernel_times.json

The scratch directory (default: a fresh temporary one) holds about 11 GB while the tool runs and is
removed afterwards."""
from __future__ import annotations

import argparse
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


def _module(model: str, n: int):
    import torch
    from tachikoma_amd import relay, zoo
    from tachikoma_amd.contrib import graph_executor
    torch.cuda.set_device(0)
    model_fn = zoo.MODELS[model]
    proto = model_fn(batch=1)

    def build_module(k):
        mdl = model_fn(batch=k)
        lib = relay.build(mdl.mod, target="mi355x", params=mdl.params)
        return graph_executor.GraphModule(lib["default"](0))

    return proto, build_module


def child_write(args) -> dict:
    """The packed chunk (through the trace job) and the unpacked dump of the same samples."""
    from tachikoma_amd import trace_job
    proto, build_module = _module(args.model, args.chunk)
    out = {}
    for packed in (True,) if args.kernel_times else (True, False):
        d = os.path.join(args.dir, "packed" if packed else "plain")
        tracer = trace_job.GraphModuleTracer(build_module, proto.sample_inputs, model=proto.name,
                                             input_name=proto.input_name, packed=packed,
                                             **({"bias": True} if packed and args.bias else {}))
        try:
            entries = trace_job.run(tracer, args.chunk, args.chunk, d, resume=False, packed=packed)
        finally:
            tracer.close()
        path = os.path.join(d, entries[0].file)
        out["packed" if packed else "plain"] = {"file": path, "bytes": os.path.getsize(path), "digest": entries[0].digest}
    return out


def child_host(args) -> dict:
    import numpy as np
    from tachikoma_amd import trace_format as tf
    t0 = time.perf_counter()
    image = tf.unpack_trace(args.packed)
    t1 = time.perf_counter()
    _, _, _, _, ro, rs = tf._header(image)
    with open(args.plain, "rb") as f:
        ref = np.fromfile(f, dtype=np.uint8, count=rs, offset=ro)
    equal = bool(np.array_equal(np.frombuffer(image, np.uint8)[ro:ro + rs], ref))
    t2 = time.perf_counter()
    return {"route": "host", "unpack_ms": (t1 - t0) * 1e3, "compare_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3,
            "equal": equal, "records_bytes": int(rs)}


def child_device(args) -> dict:
    import torch
    from tachikoma_amd import trace_format as tf
    proto, build_module = _module(args.model, args.chunk)
    gm = build_module(args.chunk)
    try:
        v = gm.trace_verifier()            # the staging and the device buffer, sized once
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = gm.verify_trace(args.packed)
        total = (time.perf_counter() - t0) * 1e3
        stats = dict(rep.stats)
        # the probe: the same pinned bytes over the link once more, nothing else in flight
        n = int(stats["upload_bytes"])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        v.device[:n].copy_(v.staging[:n], non_blocking=True)
        e1.record()
        e1.synchronize()
        probe_ms = e0.elapsed_time(e1)
        info = tf.packed_info(args.packed)
        moved = info["wire_bytes"] + info["coded_record_bytes"] + 2 * info["raw_record_bytes"]
        # a second verify: the same file again, everything warm
        t1 = time.perf_counter()
        rep2 = gm.verify_trace(args.packed)
        total2 = (time.perf_counter() - t1) * 1e3
        return {"route": "device", "total_ms": total, "ok": bool(rep.ok), "n_records": rep.n_records, "stats": stats,
                "second": {"total_ms": total2, "ok": bool(rep2.ok), "stats": dict(rep2.stats)},
                "upload_GBps": n / stats["upload_ms"] / 1e6, "probe_GBps": n / probe_ms / 1e6,
                "compare_bytes": moved, "compare_GBps": moved / stats["compare_ms"] / 1e6,
                "compare_GBps_second": moved / rep2.stats["compare_ms"] / 1e6}
    finally:
        gm.close()


def kernel_times(args, packed_file: str) -> dict:
    """One device run per tree under the profiler; the wire_decode_kernel rows of its kernel statistics."""
    import csv
    import glob
    from tachikoma_amd import trace_format as tf
    info = tf.packed_info(packed_file)
    moved = info["wire_bytes"] + info["coded_record_bytes"]
    out = {"file": {k: info[k] for k in ("version", "file_bytes", "wire_bytes", "coded_record_bytes")},
           "wire_plus_record_bytes": moved, "trees": {}}
    for i, tree in enumerate(args.tree):
        tree = os.path.abspath(tree)
        d = os.path.join(args.dir, f"rocprof_{i}")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
               os.path.join(tree, "tools", "bench_trace_verify.py"), "--child", "device", "--model", args.model,
               "--chunk", str(args.chunk), "--dir", args.dir, "--packed", packed_file]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=tree,
                           env=dict(os.environ, PYTHONPATH=tree))
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"{tree}: the profiled run failed ({r.returncode})")
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                rows += [row for row in csv.DictReader(f) if "wire_decode_kernel" in row.get("Name", "")]
        if not rows:
            raise SystemExit(f"{tree}: the profiler's kernel statistics name no wire_decode_kernel (looked under {d})")
        res = json.loads(line[7:])
        entry = {"ok": res["ok"] and res["second"]["ok"], "kernels": rows}
        for row in rows:   # compare mode is the first template argument 1
            name = row["Name"].replace(" ", "")
            if "wire_decode_kernel<1" in name or "wire_decode_kernel<(int)1" in name:
                avg = float(row["AverageNs"])
                entry["compare_avg_ms"] = avg / 1e6
                entry["compare_TBps"] = moved / avg / 1e3
        out["trees"][tree] = entry
    return out


def _spread(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model", default="resnet50")
    p.add_argument("--chunk", type=int, default=64)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--dir", default=None)
    p.add_argument("--out", default=None)
    p.add_argument("--bias", action="store_true", help="the packed chunk is a version-3 file (bias coding)")
    p.add_argument("--kernel-times", action="store_true",
                   help="profile the decode kernels alone (rocprofv3 --kernel-trace --stats, one run per --tree)")
    p.add_argument("--tree", nargs="+", default=[ROOT], help="with --kernel-times: the trees to run, each with its library built")
    p.add_argument("--child", choices=["write", "host", "device"], default=None)
    p.add_argument("--packed", default=None)
    p.add_argument("--plain", default=None)
    args = p.parse_args()
    if args.child:
        res = {"write": child_write, "host": child_host, "device": child_device}[args.child](args)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    made = args.dir is None
    args.dir = tempfile.mkdtemp(prefix="tk_verify_") if made else args.dir
    os.makedirs(args.dir, exist_ok=True)

    def run(child, *extra):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--model", args.model, "--chunk",
               str(args.chunk), "--dir", args.dir, *(["--bias"] if args.bias else []),
               *(["--kernel-times"] if args.kernel_times else []), *extra]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True)
        line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
        print(f"[bench_trace_verify] {child}: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        return json.loads(line[7:])

    try:
        files = run("write")
        if args.kernel_times:
            out = kernel_times(args, files["packed"]["file"])
            if args.out:
                with open(args.out, "w") as f:
                    f.write(json.dumps(out, indent=1) + "\n")
            print(json.dumps({t: {k: v for k, v in e.items() if k != "kernels"} for t, e in out["trees"].items()}))
            return 0
        both = ("--packed", files["packed"]["file"], "--plain", files["plain"]["file"])
        rounds = []
        for _ in range(args.rounds):
            rounds.append({"host": run("host", *both), "device": run("device", *both)})
    finally:
        if made:
            shutil.rmtree(args.dir, ignore_errors=True)
    dev = [r["device"] for r in rounds]
    out = {"model": args.model, "chunk": args.chunk, "files": files, "rounds": rounds,
           "host_total_ms": _spread([r["host"]["total_ms"] for r in rounds]),
           "host_unpack_ms": _spread([r["host"]["unpack_ms"] for r in rounds]),
           "host_compare_ms": _spread([r["host"]["compare_ms"] for r in rounds]),
           "device_total_ms": _spread([d["total_ms"] for d in dev]),
           "device_second_total_ms": _spread([d["second"]["total_ms"] for d in dev]),
           **{f"device_{k}": _spread([d["stats"][k] for d in dev]) for k in ("read_ms", "check_ms", "upload_ms", "run_ms",
                                                                              "compare_ms")},
           "upload_GBps": _spread([d["upload_GBps"] for d in dev]), "probe_GBps": _spread([d["probe_GBps"] for d in dev]),
           "compare_GBps": _spread([d["compare_GBps"] for d in dev]),
           "compare_GBps_second": _spread([d["compare_GBps_second"] for d in dev]),
           "all_equal": all(r["host"]["equal"] and r["device"]["ok"] and r["device"]["second"]["ok"] for r in rounds)}
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("rounds",)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
