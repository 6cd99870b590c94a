#!/usr/bin/env python3
"""Wire figures of the bench workload (what bench.py's line does not carry): for the traced step
of `--model` at `--batch` samples, with the trace wire on and off in one process,

  * ms per step of K back-to-back traced steps (as bench.py queues them),
  * wire bytes per step against the raw trace bytes, and the coded share (int32 records and the
    clip records coded as clamps; TK_WIRE_CLAMP=0 in the environment keeps the latter raw),
  * the wire stream's rate: bytes over the sum of the chunks' wire-work intervals
    (tk_module_copy_trace's events) -- with wire off that is the plain chunk copy rate, the
    in-run pinned-copy probe to set it against,
  * the host decode rate (image bytes written per second of decode) and the pool's thread count,
  * whether link or decoder bounds the step: the sum of the wire intervals against the sum of the
    decode times.

Prints one JSON document.  TK_WIRE_THREADS sets the decoder pool for the process."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="resnet50")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--wire-first", action="store_true", help="measure wire on before wire off")
    p.add_argument("--step-events", action="store_true",
                   help="bracket each step with timing events on the capture stream, as bench.py does")
    p.add_argument("--chunks", type=int, default=8)
    p.add_argument("--no-numa-bind", action="store_true")
    p.add_argument("--cpus", type=int, default=0,
                   help="after the binding, keep only this many CPUs of the mask (the pool then sees them)")
    args = p.parse_args()
    import torch
    import bench
    from tachikoma_amd import _lib, relay, shard, zoo
    from tachikoma_amd.contrib import graph_executor
    # as bench.py: this process (its decoder pool and pinned memory too) on the GPU's NUMA node;
    # --no-numa-bind shows what an unbound process gets
    placement = None if args.no_numa_bind else shard.bind_to_gpu_node(0)
    if args.cpus:
        os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:args.cpus])
    model = zoo.MODELS[args.model](batch=args.batch)
    lib = relay.build(model.mod, target="mi355x", params=model.params)
    table = bench.find_tune_table(args.model, args.batch)
    try:
        m = graph_executor.GraphModule(lib["default"](0, tune=table or True))
    except _lib.TachikomaError:
        m = graph_executor.GraphModule(lib["default"](0))
    m.module.use_graph = True
    _lib.check(m.module.lib.tk_module_set_trace_chunks(m.module.handle, args.chunks), "tk_module_set_trace_chunks")
    m.set_input(model.input_name, model.sample_inputs(0, args.batch))
    cap = m.trace_capture()
    stream = torch.cuda.current_stream()
    raw = sum(op.out.nbytes for op in m.plan.ops)

    evs = []

    def step():
        cap.capture_stream.wait_stream(stream)
        if args.step_events:
            evs.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            evs[-1][0].record(cap.capture_stream)
        cap.capture_inputs(stream)
        m.module.run(stream, cap.capture_stream, cap.host_dst)
        if args.step_events:
            evs[-1][1].record(cap.capture_stream)

    out = {"model": args.model, "batch": args.batch, "record_bytes_per_step": raw,
           "placement": placement and {k: placement[k] for k in ("numa_node", "cpus", "bound")},
           "cpus_in_mask": len(os.sched_getaffinity(0)), "library": _lib.build_info(),
           "decoder_threads": _lib.load().tk_wire_threads(), "modes": {}}
    ref = None
    for wire in ((True, False, True, False) if args.wire_first else (False, True, False, True)):
        m.module.set_trace_wire(wire)
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        img = bytes(cap.bytes())
        ref = img if ref is None else ref   # (both modes give the same image, whichever ran first)
        m.module.set_copy_trace(True)
        step()
        torch.cuda.synchronize()
        ct = m.module.copy_trace()
        ws = m.module.wire_stats()
        m.module.set_copy_trace(False)
        busy = sum(c["end_ms"] - c["start_ms"] for c in ct)
        t1 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        r = {"ms_per_step": round(ms, 2), "image_equals_wire_off": img == ref,
             "single_step_ms": round((time.perf_counter() - t1) * 1e3, 2),
             "stream_busy_ms": round(busy, 2),
             "stream_span_ms": round(ct[-1]["end_ms"] - ct[0]["start_ms"], 2) if ct else None}
        if wire:
            wb = sum(s["wire_bytes"] for s in ws)
            coded = sum(s["coded_raw_bytes"] for s in ws)
            dec = sum(s["decode_ms"] for s in ws)
            r.update(wire_bytes_per_step=wb, wire_over_raw=round(wb / raw, 4), coded_raw_bytes=coded,
                     wire_stream_GBps=round(wb / (busy * 1e-3) / 1e9, 2), decode_ms=round(dec, 2),
                     decode_GBps=round(coded / (dec * 1e-3) / 1e9, 2) if dec else None,
                     decode_ms_per_chunk=[round(s["decode_ms"], 2) for s in ws],
                     bound_by="decoder" if dec > busy else "link")
        else:
            r.update(copy_GBps=round(sum(c["bytes"] for c in ct) / (busy * 1e-3) / 1e9, 2))
        out["modes"].setdefault("wire_on" if wire else "wire_off", []).append(r)
    m.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
