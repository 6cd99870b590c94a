"""relay.quantize's dataset calibration on one GPU: the host path against the device path.

In one process, interleaved rounds of, per calibrate mode (kl_divergence, percentile),

  host     collect_stats + find_scale_by_kl / find_scale_by_percentile (device_stats=False): every
           profiled activation of every batch copied to the host and reduced in numpy;
  device   device_scales (device_stats=True): ranges + histogram, or three digit passes, where the
           activations lie;

with the wall time of each (both build the profile graph once, inside the timed part), the graph
runs, the bytes copied to the host and a check that the scales are equal.  Then, on the profile
graph's records after one run, the three kernels' times from HIP events, each against a streaming
read (torch.sum) of a buffer of the same bytes measured in the same run.

--remedy takes the A/B of the histogram pass's contention remedy at the kernel level instead: a
ReLU-shaped synthetic record (half exact zeros), the four combinations of "zeros in registers"
and "whole-lane add", each in a process of its own on the profiling build of the library
(tachikoma_amd/build.py --ablation, TK_FSTATS_REMEDY; the product library has the zeros in
registers only, which is what this A/B kept).

--device-kl measures the threshold search on the device (device_scales(..., device_kl=True),
csrc/tk_kl.hip) against the device_stats=True path of the parent commit, whose tree --parent-tree
names (an export of that commit with its library built): interleaved child processes, one per
tree, each one warm-up call and --rounds timed ones.  Then, on this tree, the evaluate and the
select kernel from HIP events over the histograms of the profile graph, the survivors per layer,
the fallbacks and the largest part of the bound that the host's divergences use.

    python tools/bench_calibrate.py --out profiles/device_calibration_resnet18.json
    python tools/bench_calibrate.py --remedy --out profiles/device_calibration_remedy.json
    python tools/bench_calibrate.py --device-kl --parent-tree DIR --out profiles/device_kl_resnet18.json"""
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

REPS = 5


def _spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _annotated(m):
    from tachikoma_amd.relay.quantize import passes
    return passes.annotate(passes.partition(passes.prerequisite_optimize(m.mod, m.params)))


def end_to_end(args) -> dict:
    import numpy as np
    from tachikoma_amd import zoo
    from tachikoma_amd.contrib import graph_executor, trace_device
    from tachikoma_amd.relay.quantize import passes, qconfig

    m = zoo.resnet_float(args.depth, batch=args.batch, hw=args.hw)
    mod = _annotated(m)
    data = [{"data": m.random_input(seed=s)} for s in range(args.batches)]
    meter = {"runs": 0, "bytes": 0}
    run, get = graph_executor.GraphModule.run, graph_executor.GraphModule.get_node_output
    down = trace_device.FloatStatsAccumulator._download

    def counted_run(self, *a, **k):
        meter["runs"] += 1
        return run(self, *a, **k)

    def counted_get(self, name):
        view = get(self, name)
        buf = self.module.buffers[name]
        meter["bytes"] += buf.numel() * buf.element_size()
        return view

    def counted_down(self, dev, stream):
        meter["bytes"] += dev.numel() * dev.element_size()
        return down(self, dev, stream)

    graph_executor.GraphModule.run = counted_run
    graph_executor.GraphModule.get_node_output = counted_get
    trace_device.FloatStatsAccumulator._download = counted_down
    rows = {}
    try:
        for mode in ("kl_divergence", "percentile"):
            finder = passes.find_scale_by_kl if mode == "kl_divergence" else passes.find_scale_by_percentile
            paths = {"host": lambda: passes._dataset_scales(mod, data, finder),
                     "device": lambda: passes.device_scales(mod, data, mode)}
            got = {k: {"wall_s": []} for k in paths}
            with qconfig(calibrate_mode=mode):
                for rnd in range(args.rounds + 1):  # the first round warms both paths up and is dropped
                    for name, fn in paths.items():
                        meter["runs"] = meter["bytes"] = 0
                        t0 = time.perf_counter()
                        scales = fn()
                        wall = time.perf_counter() - t0
                        if rnd:
                            got[name]["wall_s"].append(wall)
                        got[name].update(graph_runs=meter["runs"], bytes_to_host=meter["bytes"], scales=scales)
                        print(f"[bench_calibrate] {mode} {name} round {rnd}: {wall:.2f} s", file=sys.stderr, flush=True)
            equal = (np.array(got["host"].pop("scales"), np.float64).tobytes() ==
                     np.array(got["device"].pop("scales"), np.float64).tobytes())
            for v in got.values():
                v["wall_s_spread"] = _spread(v["wall_s"])
            rows[mode] = {**got, "scales_equal": equal, "layers": len(passes.stats_profile(mod)[1]),
                          "host_over_device": round(statistics.median(got["host"]["wall_s"]) /
                                                    statistics.median(got["device"]["wall_s"]), 3)}
    finally:
        graph_executor.GraphModule.run, graph_executor.GraphModule.get_node_output = run, get
        trace_device.FloatStatsAccumulator._download = down
    return rows


def kernels(args) -> dict:
    """The three passes over the profile graph's float32 records after one run, HIP-event timed."""
    import torch
    from tachikoma_amd import relay, zoo
    from tachikoma_amd.contrib import graph_executor
    from tachikoma_amd.relay.quantize import passes

    m = zoo.resnet_float(args.depth, batch=args.batch, hw=args.hw)
    prof, _ = passes.stats_profile(_annotated(m))
    gm = graph_executor.GraphModule(relay.build(prof, target="mi355x")["default"]())
    try:
        gm.run(data=m.random_input(seed=0))
        graph_ms = [_timed(gm.run) for _ in range(REPS)]
        acc = gm.float_stats_accumulator()
        bufs = gm.module.buffers
        nbytes = sum(bufs[n].numel() * 4 for n in acc.names)
        zeros = sum(int((bufs[n] == 0).sum().item()) for n in acc.names)
        acc.add_range()
        acc.set_edges(8001)
        flat = torch.randn(nbytes // 4, device=gm.module.device)
        out = {"records": len(acc.names), "read_bytes": nbytes, "zero_fraction": round(zeros / (nbytes // 4), 4),
               "profile_graph_run_ms": _spread(graph_ms)}
        steps = {"range": acc.add_range, "histogram": acc.add_histogram, "digits": lambda: acc.add_digits(0),
                 "streaming_read": lambda: torch.sum(flat)}
        ms = {k: [] for k in steps}
        for fn in steps.values():
            fn()
        for _ in range(REPS):  # interleaved
            for k, fn in steps.items():
                ms[k].append(_timed(fn))
        ref = statistics.median(ms["streaming_read"])
        for k, v in ms.items():
            med = statistics.median(v)
            out[k] = {"ms": _spread(v), "GBps": round(nbytes / med / 1e6, 1),
                      "of_streaming_read_rate": round(ref / med, 3)}
        return out
    finally:
        gm.close()


def child_remedy(args) -> dict:
    """One variant of the histogram pass on a ReLU-shaped record of args.elements float32."""
    import numpy as np
    import torch
    from tachikoma_amd import _lib
    from tachikoma_amd.relay.quantize import passes
    lib = _lib.load()
    torch.cuda.set_device(0)
    n = int(args.elements)
    x = torch.relu(torch.randn(n, device="cuda", generator=torch.Generator("cuda").manual_seed(1)))
    lo, hi = float(x.min().item()), float(x.max().item())
    edges = torch.from_numpy(passes.histogram_edges(np.float32(lo), np.float32(hi), 8001)).cuda()
    hist = torch.zeros(8001, dtype=torch.int64, device="cuda")
    plan = ctypes.c_void_p()
    _lib.check(lib.tk_fstats_plan_create((ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_int64 * 1)(n), 1,
                                         ctypes.byref(plan)), "tk_fstats_plan_create")
    s = ctypes.c_void_p(_lib.stream_handle(None))
    run = lambda: _lib.check(lib.tk_fstats_plan_histogram(plan, ctypes.c_void_p(edges.data_ptr()), 8001,  # noqa: E731
                                                          ctypes.c_void_p(hist.data_ptr()), s), "histogram")
    first = _timed(run)
    ms = [_timed(run) for _ in range(REPS)]
    read = [_timed(lambda: torch.sum(x)) for _ in range(REPS + 1)][1:]
    lib.tk_fstats_plan_destroy(plan)
    total = int(hist.sum().item())
    assert total == (REPS + 1) * n, (total, n)
    med = statistics.median(ms)
    return {"remedy": int(os.environ.get("TK_FSTATS_REMEDY", "1")), "library": _lib.build_info(), "elements": n,
            "zero_fraction": round(float((x == 0).float().mean().item()), 4), "first_ms": round(first, 3),
            "ms": _spread(ms), "GBps": round(4 * n / med / 1e6, 1),
            "streaming_read_ms": _spread(read), "of_streaming_read_rate": round(statistics.median(read) / med, 3)}


def remedy(args) -> dict:
    from tachikoma_amd import build
    lib = build.build_ablation(verbose=False)
    names = {0: "neither", 1: "zeros in registers", 2: "whole-lane add", 3: "both"}
    rows = {v: [] for v in names.values()}
    for _ in range(args.rounds):
        for bits, name in names.items():
            env = dict(os.environ, TK_LIB_PATH=lib, TK_FSTATS_REMEDY=str(bits))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-remedy", "--elements",
                                str(args.elements)], stdout=subprocess.PIPE, text=True, check=True, env=env, timeout=120)
            rows[name].append(json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:]))
    return {"record": "relu(normal), float32", "elements": int(args.elements), "bins": 8001,
            "variants": {k: {"ms_median_of_rounds": _spread([r["ms"]["median"] for r in v]),
                             "of_streaming_read_rate": _spread([r["of_streaming_read_rate"] for r in v]),
                             "zero_fraction": v[0]["zero_fraction"], "rounds": v} for k, v in rows.items()}}


def child_e2e(args) -> dict:
    """kl_divergence scales of one variant, in the tree this process imports: one warm-up call and
    args.rounds timed ones."""
    import numpy as np
    from tachikoma_amd import _lib, zoo
    from tachikoma_amd.relay.quantize import passes, qconfig
    m = zoo.resnet_float(args.depth, batch=args.batch, hw=args.hw)
    mod = _annotated(m)
    data = [{"data": m.random_input(seed=s)} for s in range(args.batches)]
    kw = {"device_kl": True} if args.child_e2e == "device_kl" else {}
    wall, scales = [], None
    with qconfig(calibrate_mode="kl_divergence"):
        for rnd in range(args.rounds + 1):
            t0 = time.perf_counter()
            scales = passes.device_scales(mod, data, "kl_divergence", **kw)
            if rnd:
                wall.append(time.perf_counter() - t0)
    return {"variant": args.child_e2e, "library": _lib.build_info(), "wall_s": wall, "layers": len(scales),
            "scales_hex": np.array(scales, np.float64).tobytes().hex()}


def kl_kernels(args) -> dict:
    """The two kernels of tk_kl_device over the histograms of the profile graph (HIP events), and
    what the search came to per layer against the host's own divergences."""
    import numpy as np
    import torch
    from tachikoma_amd import _lib, relay, zoo
    from tachikoma_amd.contrib import graph_executor, trace_device
    from tachikoma_amd.relay.quantize import passes

    m = zoo.resnet_float(args.depth, batch=args.batch, hw=args.hw)
    mod = _annotated(m)
    prof, targets = passes.stats_profile(mod)
    gm = graph_executor.GraphModule(relay.build(prof, target="mi355x")["default"]())
    try:
        names, counter = {}, 0
        for n in relay.post_order(prof["main"].body):
            if isinstance(n, relay.Call):
                names[id(n)] = f"%{counter}"
                counter += 1
            elif isinstance(n, relay.Var):
                names[id(n)] = n.name_hint
        uniq = list(dict.fromkeys(names[id(t)] for t in targets))
        acc = gm.float_stats_accumulator(uniq)
        data = [m.random_input(seed=s) for s in range(args.batches)]
        for x in data:
            gm.run(data=x)
            acc.add_range()
        acc.set_edges(8001)
        for x in data:
            gm.run(data=x)
            acc.add_histogram()
        bins, nq = 8001, 255
        t0 = time.perf_counter()
        found = acc.kl_thresholds(nq)
        search_s = time.perf_counter() - t0
        picks, table = acc.kl_picks, acc.kl_table()
        lib, n = gm.module.lib, len(uniq)
        s = ctypes.c_void_p(_lib.stream_handle(None))
        hist, tab = ctypes.c_void_p(acc._hist.data_ptr()), ctypes.c_void_p(acc._kl_table.data_ptr())
        pk = torch.empty(n * trace_device.KL_PICK_DTYPE.itemsize // 8, dtype=torch.int64, device=gm.module.device)
        steps = {"evaluate": lambda: _lib.check(lib.tk_kl_device_evaluate(hist, n, bins, nq, tab, s), "evaluate"),
                 "select": lambda: _lib.check(lib.tk_kl_device_select(hist, n, bins, nq, tab, ctypes.c_void_p(pk.data_ptr()), s),
                                              "select")}
        ms = {k: [_timed(fn) for _ in range(REPS)] for k, fn in steps.items()}
        counts = acc.histograms()
        used, host_s, equal = 0.0, 0.0, True
        for name in uniq:
            h, edges = counts[name]
            t0 = time.perf_counter()
            host = trace_device.kl_candidates(h, bins, nq, np.arange(table[name].size))
            host_s += time.perf_counter() - t0
            fin = np.isfinite(host["div"])
            err = np.abs(host["div"][fin].astype(np.float64) - table[name]["d"][fin])
            used = max(used, float((err / table[name]["bound"][fin]).max()))
            want = float(edges[bins // 2 + nq // 2 + int(np.argmin(host["div"])) + 1])
            equal = equal and np.float32(want).tobytes() == np.float32(found[name]).tobytes()
        return {"layers": n, "bins": bins, "quantized_bins": nq, "candidates_per_layer": int(table[uniq[0]].size),
                "evaluate_ms": _spread(ms["evaluate"]), "select_ms": _spread(ms["select"]),
                "kl_thresholds_wall_s": round(search_s, 4), "host_all_candidates_s": round(host_s, 3),
                "survivors_per_layer": [int(c) for c in picks["count"]], "statuses": [int(c) for c in picks["status"]],
                "fallbacks": len(acc.kl_fallbacks), "largest_bound_fraction_used": round(used, 4),
                "thresholds_equal_host_argmin": bool(equal)}
    finally:
        gm.close()


def device_kl(args) -> dict:
    script = os.path.abspath(__file__)
    trees = {"device_stats_parent": (args.parent_tree, "device"), "device_kl": (ROOT, "device_kl")}
    rows = {k: [] for k in trees}
    for _ in range(2):  # interleaved: parent, this tree, parent, this tree
        for name, (tree, variant) in trees.items():
            r = subprocess.run([sys.executable, script, "--child-e2e", variant, "--tree", tree, "--depth", str(args.depth),
                                "--batch", str(args.batch), "--hw", str(args.hw), "--batches", str(args.batches),
                                "--rounds", str(args.rounds)], stdout=subprocess.PIPE, text=True, check=True, timeout=600)
            rows[name].append(json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:]))
            print(f"[bench_calibrate] {name}: {rows[name][-1]['wall_s']}", file=sys.stderr, flush=True)
    out = {}
    for name, rs in rows.items():
        wall = [w for r in rs for w in r["wall_s"]]
        out[name] = {"library": rs[0]["library"], "wall_s": [round(w, 3) for w in wall], "wall_s_spread": _spread(wall),
                     "layers": rs[0]["layers"]}
    out["scales_equal"] = len({r["scales_hex"] for rs in rows.values() for r in rs}) == 1
    out["parent_over_device_kl"] = round(out["device_stats_parent"]["wall_s_spread"]["median"] /
                                         out["device_kl"]["wall_s_spread"]["median"], 3)
    return out


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--depth", type=int, default=18)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--hw", type=int, default=224)
    p.add_argument("--batches", type=int, default=2, help="batches of the calibration dataset")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--elements", default=str(1 << 26), help="--remedy: float32 elements of the synthetic record")
    p.add_argument("--remedy", action="store_true")
    p.add_argument("--child-remedy", action="store_true")
    p.add_argument("--device-kl", action="store_true")
    p.add_argument("--parent-tree", default=None, help="--device-kl: the parent commit's tree, library built")
    p.add_argument("--child-e2e", default=None, choices=["device", "device_kl"])
    p.add_argument("--tree", default=None, help="--child-e2e: the tree to import tachikoma_amd from")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.child_e2e:
        sys.path.insert(0, os.path.abspath(args.tree or ROOT))
        print("RESULT " + json.dumps(child_e2e(args)), flush=True)
        return 0
    if args.child_remedy:
        print("RESULT " + json.dumps(child_remedy(args)), flush=True)
        return 0
    if args.device_kl:
        if not args.parent_tree:
            p.error("--device-kl needs --parent-tree")
        out = {"model": f"resnet{args.depth}_float", "batch": args.batch, "hw": args.hw, "dataset_batches": args.batches,
               "rounds_per_process": args.rounds, "end_to_end_kl_divergence": device_kl(args), "kernels": kl_kernels(args),
               "counter_run": False}
    elif args.remedy:
        out = {"contention_remedy": remedy(args)}
    else:
        out = {"model": f"resnet{args.depth}_float", "batch": args.batch, "hw": args.hw, "dataset_batches": args.batches,
               "rounds": args.rounds, "end_to_end": end_to_end(args), "kernels": kernels(args), "counter_run": False}
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
