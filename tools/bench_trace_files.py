"""Chunk-file throughput of the trace job, packed against unpacked against another tree's.

Traces a model (ResNet-50) in chunks of 64 samples, at least 6 chunks per run, into one directory,
in three interleaved rounds of (the parent tree's trace job, this tree unpacked, this tree packed),
each run in a fresh process.  A chunk's time is the interval between two consecutive journal
entries (a chunk is journalled when its file is complete on disk), so the first chunk, which
carries the module build and the find step, is left out.  Reported per mode: ms per chunk (median,
min-max over all rounds), bytes per chunk file, and for the packed mode the packer's time (the
tk_wire_pack_device call, after the run is complete), the copy into the pinned staging, the file
write, and what trace_format.unpack_trace needs for one chunk file.  One round also checks that a
packed chunk unpacks to the very file the unpacked job wrote and that the journal digests agree.

    python tools/bench_trace_files.py --parent-tree DIR --dir SCRATCH --out profiles/packed_trace_files_resnet50.json

DIR holds the parent commit's ``tachikoma_amd`` package (with its library built) and ``oracle``;
without it the parent mode is left out.  A chunk file is deleted once the next one is journalled,
the last one after the run.

With ``--modes`` the arms are chosen by name (default: parent, unpacked, packed): ``parent_packed`` is
the parent tree's packed job, ``packed_bias`` this tree's ``--packed --bias-coding`` (format version
3).  The three-arm run of the version-3 files is

    python tools/bench_trace_files.py --parent-tree DIR --dir SCRATCH --modes parent_packed packed packed_bias \
        --out profiles/packed_bias_trace_job_resnet50.json"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(args) -> int:
    """One trace job in this process, from the package under --tree; prints one JSON line."""
    sys.path.insert(0, args.tree)
    import torch
    from tachikoma_amd import relay, trace_job, zoo
    from tachikoma_amd.contrib import graph_executor
    assert os.path.dirname(os.path.dirname(os.path.abspath(trace_job.__file__))) == os.path.abspath(args.tree)
    packed = args.child in ("packed", "parent_packed", "packed_bias")
    stamps, sizes = [], []
    append = trace_job.Journal.append
    import concurrent.futures
    cleaner = concurrent.futures.ThreadPoolExecutor(max_workers=1)

    def stamped(self, entry):
        append(self, entry)
        stamps.append(time.perf_counter())
        sizes.append(entry["bytes"])
        if entry["chunk"] > 0:   # only the newest file is kept (off this thread): 6 x 7.45 GB need not fit the disk
            cleaner.submit(os.remove, trace_job.chunk_file(args.dir, 0, entry["chunk"] - 1))

    trace_job.Journal.append = stamped
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    model_fn = zoo.MODELS[args.model]
    proto = model_fn(batch=1)

    def build_module(n):
        mdl = model_fn(batch=n)
        lib = relay.build(mdl.mod, target="mi355x", params=mdl.params)
        return graph_executor.GraphModule(lib["default"](device.index))

    kw = {"packed": True} if packed else {}
    tracer = trace_job.GraphModuleTracer(build_module, proto.sample_inputs, model=proto.name,
                                         input_name=proto.input_name, **kw,
                                         **({"bias": True} if args.child == "packed_bias" else {}))
    t0 = time.perf_counter()
    try:
        entries = trace_job.run(tracer, args.chunks * args.chunk, args.chunk, args.dir, resume=False, **kw)
    finally:
        tracer.close()
        cleaner.shutdown(wait=True)
    files = [os.path.join(args.dir, e.file) for e in entries]
    out = {"mode": args.child, "first_chunk_ms": (stamps[0] - t0) * 1e3,
           "chunk_ms": [(b - a) * 1e3 for a, b in zip(stamps, stamps[1:])],
           "file_bytes": sizes, "digests": [e.digest for e in entries]}
    if packed:
        from tachikoma_amd import trace_format as tf
        for k in ("pack_ms", "copy_ms", "write_ms"):
            out[k] = [s[k] for s in tracer.stats[1:]]
        with open(files[-1], "rb") as f:
            out["file_version"] = int.from_bytes(f.read(16)[8:], "little")
        t1 = time.perf_counter()
        image = tf.unpack_trace(files[-1])
        out["unpack_ms"] = (time.perf_counter() - t1) * 1e3
        out["unpacked_bytes"] = len(image)
        if args.compare_with and os.path.exists(args.compare_with):
            with open(args.compare_with, "rb") as f:
                out["unpacks_to_the_unpacked_file"] = image == f.read()
            out["compared_chunk"] = os.path.basename(files[-1])
    print("RESULT " + json.dumps(out), flush=True)
    return 0


def _spread(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2), "n": len(xs)}


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model", default="resnet50")
    p.add_argument("--chunk", type=int, default=64)
    p.add_argument("--chunks", type=int, default=6)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--dir", required=True, help="scratch directory for the chunk files (emptied after every run)")
    p.add_argument("--parent-tree", default=None, help="the parent commit's package, built")
    p.add_argument("--modes", nargs="+", default=None,
                   choices=["parent", "parent_packed", "unpacked", "packed", "packed_bias"],
                   help="the arms of a round, in order (default: parent, unpacked, packed)")
    p.add_argument("--out", default=None, help="write the report (JSON) here")
    p.add_argument("--timeout", type=int, default=600, help="seconds one run may take")
    p.add_argument("--append-to", default=None,
                   help="an earlier report of the same settings: its rounds come first (rounds split over invocations)")
    p.add_argument("--child", default=None, help=argparse.SUPPRESS)
    p.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    p.add_argument("--compare-with", default=None, help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.child:
        return child(args)
    if args.chunks < 2:
        p.error("--chunks must be at least 2 (the first chunk is not timed)")
    names = args.modes or ["parent", "unpacked", "packed"]
    modes = [(m, args.parent_tree if m.startswith("parent") else ROOT) for m in names
             if args.parent_tree or not m.startswith("parent")]
    packed_modes = ("packed", "parent_packed", "packed_bias")
    compared = next((m for m in names if m in packed_modes), None) if "unpacked" in names else None
    os.makedirs(args.dir, exist_ok=True)
    kept = os.path.join(args.dir, "kept_unpacked_chunk.tkt")
    st = os.statvfs(args.dir)
    report = {"model": args.model, "chunk": args.chunk, "chunks_per_run": args.chunks, "rounds": [],
              "scratch_free_gb": round(st.f_bavail * st.f_frsize / 1e9, 1)}
    first = 0
    if args.append_to:
        with open(args.append_to) as f:
            before = json.load(f)
        assert (before["model"], before["chunk"], before["chunks_per_run"]) == (args.model, args.chunk, args.chunks)
        report["rounds"] = before["rounds"]
        first = len(before["rounds"])
    for r in range(first, first + args.rounds):
        this = {}
        for mode, tree in modes:
            run_dir = os.path.join(args.dir, f"r{r}_{mode}")
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--tree", os.path.abspath(tree),
                   "--dir", run_dir, "--model", args.model, "--chunk", str(args.chunk), "--chunks", str(args.chunks)]
            if mode == compared and r == first:
                cmd += ["--compare-with", kept]
            env = dict(os.environ, PYTHONPATH=os.path.abspath(tree))
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, env=env, cwd=tree)
            line = next((ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")), None)
            if res.returncode != 0 or line is None:
                sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
                shutil.rmtree(args.dir, ignore_errors=True)
                raise SystemExit(f"round {r} mode {mode}: the trace job failed ({res.returncode})")
            this[mode] = json.loads(line[7:])
            if mode == "unpacked" and r == first:   # the last chunk, for the packed run of this round to compare with
                os.replace(os.path.join(run_dir, f"trace.rank0.chunk{args.chunks - 1}.tkt"), kept)
            shutil.rmtree(run_dir, ignore_errors=True)
            print(f"round {r} {mode}: {_spread(this[mode]['chunk_ms'])} ms/chunk, "
                  f"{this[mode]['file_bytes'][0]} bytes/chunk", file=sys.stderr, flush=True)
        if r == first and os.path.exists(kept):
            os.remove(kept)
        report["rounds"].append(this)
    summary = {}
    for mode, _ in modes:
        runs = [rd[mode] for rd in report["rounds"]]
        s = {"ms_per_chunk": _spread([x for run in runs for x in run["chunk_ms"]]),
             "ms_per_chunk_by_round": [_spread(run["chunk_ms"]) for run in runs],
             "bytes_per_chunk_file": _spread([x for run in runs for x in run["file_bytes"]])}
        if mode in packed_modes:
            for k in ("pack_ms", "copy_ms", "write_ms"):
                s[k] = _spread([x for run in runs for x in run[k]])
            s["unpack_ms_one_chunk"] = _spread([run["unpack_ms"] for run in runs])
            s["file_version"] = sorted({run["file_version"] for run in runs})
            if any("unpacks_to_the_unpacked_file" in run for run in runs):
                s["unpacks_to_the_unpacked_file"] = all(run["unpacks_to_the_unpacked_file"] for run in runs
                                                        if "unpacks_to_the_unpacked_file" in run)
        summary[mode] = s
    if "unpacked" in summary and "packed" in summary:
        summary["packed_over_unpacked_bytes"] = round(summary["packed"]["bytes_per_chunk_file"]["median"] /
                                                      summary["unpacked"]["bytes_per_chunk_file"]["median"], 4)
        summary["journal_digests_equal"] = all(rd["packed"]["digests"] == rd["unpacked"]["digests"]
                                               for rd in report["rounds"])
    have = [m for m, _ in modes if m in packed_modes]
    if len(have) > 1:   # the packed arms agree on the records, whatever the coding
        summary["packed_journal_digests_equal"] = all(rd[m]["digests"] == rd[have[0]]["digests"]
                                                      for rd in report["rounds"] for m in have)
        if "packed_bias" in summary and "packed" in summary:
            summary["bias_over_packed_bytes"] = round(summary["packed_bias"]["bytes_per_chunk_file"]["median"] /
                                                      summary["packed"]["bytes_per_chunk_file"]["median"], 4)
    report["summary"] = summary
    text = json.dumps(report, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(summary, indent=1))
    shutil.rmtree(args.dir, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
