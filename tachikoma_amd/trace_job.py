"""Resumable trace generation over a dataset larger than one batch (SURVEY.md §5,
"checkpoint / resume": the reference has no trace resume; samples are independent,
python/tvm/mrt/trace.py:65-117, so a shard is resumable per batch index).

A rank's shard of the global sample range (``shard.shard_range``) is cut into chunks of
``chunk`` samples; chunk c is traced as one batch and written to its own trace file
``<stem>.rank<r>.chunk<c>.tkt`` whose header carries the chunk's ``sample_offset``.  A
chunk counts as done only once its file is complete on disk: the file is written under a
``.partial`` name, fsync'd and renamed, and then one JSON line
``{"chunk", "sample_offset", "n_samples", "file", "bytes", "digest", "packed"}`` is appended (and
fsync'd) to the rank's journal ``<stem>.rank<r>.journal``.  A restarted job replays the
journal, keeps the chunks whose entry matches the plan and whose file still has the
recorded size (and, with ``verify``, the recorded record digest), and traces the rest.  A
crash at any point therefore loses at most the chunks in flight.

With ``packed`` the chunk files are packed (version 2) trace files (trace_format.pack_trace /
unpack_trace): same names, same manifest, same digests (the digest is of the records, not of the
file), about half the bytes.  ``"packed"`` in a journal entry says which kind the file is, and a
resumed job re-traces the chunks whose flag differs from its own.  With ``packed`` and ``bias``
(``--packed --bias-coding``) they are version-3 files, which also carry the wire's bias coding and
the addends it needs (about a seventh smaller on ResNet-50); the entry then adds ``"version": 3``,
and entries without the field are version 2 (packed) or 1.  Every reader takes all three versions.

With ``stats`` every chunk's records are also reduced on the device to per-record statistics
(GraphModule.stats_accumulator), written beside the chunk file as ``<chunk file>.stats.json`` before
the chunk is journalled, and :func:`merge_stats` merges the journalled chunks' statistics into
``<stem>.rank<r>.stats.json``; the journal itself does not change.  ``--stats-only`` writes only that
merged file: compute-only runs, no chunk files, no journal, not resumable.

On the device the chunk files are produced by :class:`GraphModuleTracer`: two pinned trace
images alternate, so chunk c's file is written by a host thread while chunk c+1 runs and
its records are copied D2H (the bench's file sink, overlapped with the next batch).  With
``packed`` two device packers with their pinned stagings alternate instead (PackedCapture).

CLI (one process per GPU, torch.distributed.run environment; rank 0 writes the manifest)::

    python -m tachikoma_amd.trace_job --model resnet50 --samples 4096 --chunk 64 --out-dir DIR [--packed [--bias-coding]]

``--check`` traces nothing: it walks the rank's journal and verifies every chunk file against the
engine on the device, record by record (:func:`check`, GraphModule.verify_trace), printing one JSON
line per chunk; ``--verify`` keeps its meaning (re-digest the files a resumed job keeps).  ``--check
--replay`` re-executes every op of each chunk from its recorded inputs instead
(GraphModule.replay_trace) and adds the faulty nodes and the faulty ops to the chunk's JSON line.
"""
from __future__ import annotations

import argparse
import concurrent.futures
import json
import os
import sys
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

from . import shard
from . import trace_format as tf

JOURNAL_FORMAT = "tachikoma-trace-journal"


@dataclass(frozen=True)
class Chunk:
    index: int
    sample_offset: int
    n_samples: int
    file: str


def chunk_file(out_dir: str, rank: int, index: int, stem: str = "trace") -> str:
    return os.path.join(out_dir, f"{stem}.rank{rank}.chunk{index}.tkt")


def journal_file(out_dir: str, rank: int, stem: str = "trace") -> str:
    return os.path.join(out_dir, f"{stem}.rank{rank}.journal")


def plan_chunks(global_samples: int, world: int, rank: int, chunk: int, out_dir: str,
                stem: str = "trace") -> List[Chunk]:
    """This rank's contiguous shard cut into chunks of ``chunk`` samples (the last one may be
    shorter); chunk indices are per rank."""
    if chunk <= 0:
        raise ValueError("chunk must be positive")
    off, n = shard.shard_range(global_samples, world, rank)
    out = []
    for i, s in enumerate(range(0, n, chunk)):
        out.append(Chunk(i, off + s, min(chunk, n - s), chunk_file(out_dir, rank, i, stem)))
    return out


def _fsync_dir(path: str) -> None:
    try:
        fd = os.open(os.path.dirname(os.path.abspath(path)) or ".", os.O_RDONLY)
    except OSError:
        return
    try:
        os.fsync(fd)
    except OSError:
        pass
    finally:
        os.close(fd)


class Journal:
    """Append-only JSON-lines record of the chunks whose files are complete."""

    def __init__(self, path: str):
        self.path = path

    def entries(self) -> Dict[int, dict]:
        """chunk index → last entry; a torn last line (crash during append) is ignored."""
        out: Dict[int, dict] = {}
        try:
            with open(self.path) as f:
                lines = f.read().split("\n")
        except FileNotFoundError:
            return out
        for ln in lines:
            if not ln.strip():
                continue
            try:
                e = json.loads(ln)
            except json.JSONDecodeError:
                continue
            if e.get("format") == JOURNAL_FORMAT and isinstance(e.get("chunk"), int):
                out[e["chunk"]] = e
        return out

    def append(self, entry: dict) -> None:
        line = json.dumps(dict(entry, format=JOURNAL_FORMAT), separators=(",", ":")) + "\n"
        with open(self.path, "a") as f:
            f.write(line)
            f.flush()
            os.fsync(f.fileno())

    def reset(self) -> None:
        if os.path.exists(self.path):
            os.remove(self.path)


def _valid(entry: dict, c: Chunk, verify: bool, packed: bool = False, version: Optional[int] = None) -> bool:
    if (entry.get("sample_offset"), entry.get("n_samples"), entry.get("file")) != (c.sample_offset, c.n_samples,
                                                                                     os.path.basename(c.file)):
        return False
    if bool(entry.get("packed", False)) != packed:  # entries from before the flag are unpacked files
        return False
    if version is not None and entry.get("version", 2 if entry.get("packed") else 1) != version:
        return False
    try:
        if os.path.getsize(c.file) != entry.get("bytes"):
            return False
    except OSError:
        return False
    if verify:
        try:
            return shard.hex64(tf.trace_file_digest(c.file)) == entry.get("digest")
        except (OSError, ValueError):
            return False
    return True


# A tracer takes (sample_offset, n_samples, path) and returns a Future that resolves to the
# u64 record digest once ``path`` holds the complete trace file of those samples.
Tracer = Callable[[int, int, str], "concurrent.futures.Future[int]"]


def run(tracer: Tracer, global_samples: int, chunk: int, out_dir: str, rank: int = 0, world: int = 1,
        resume: bool = True, verify: bool = False, stem: str = "trace",
        log: Optional[Callable[[str], None]] = None, packed: Optional[bool] = None) -> List[shard.ShardEntry]:
    """Trace this rank's chunks that are not done yet; returns the entries of ALL its chunks
    (resumed and new) in sample order.  ``packed``: whether the tracer writes packed files (default:
    the tracer's own ``packed`` attribute, else False); it is journalled, and chunks journalled with
    the other value are traced again."""
    packed = bool(getattr(tracer, "packed", False) if packed is None else packed)
    version = getattr(tracer, "file_version", None)  # a tracer that says which version it writes: journalled too
    os.makedirs(out_dir, exist_ok=True)
    chunks = plan_chunks(global_samples, world, rank, chunk, out_dir, stem)
    journal = Journal(journal_file(out_dir, rank, stem))
    if not resume:
        journal.reset()
    done = journal.entries() if resume else {}
    kept = {c.index: done[c.index] for c in chunks if c.index in done and _valid(done[c.index], c, verify, packed, version)}
    todo = [c for c in chunks if c.index not in kept]
    if log:
        log(f"rank {rank}: {len(chunks)} chunks, {len(kept)} done, {len(todo)} to trace")
    pending: List = []

    def finish(c: Chunk, fut) -> None:
        digest = int(fut.result()) & 0xFFFFFFFFFFFFFFFF
        tmp = c.file + ".partial"
        with open(tmp, "rb+") as f:
            os.fsync(f.fileno())
        os.replace(tmp, c.file)
        _fsync_dir(c.file)
        e = {"chunk": c.index, "sample_offset": c.sample_offset, "n_samples": c.n_samples,
             "file": os.path.basename(c.file), "bytes": os.path.getsize(c.file), "digest": shard.hex64(digest), "packed": packed}
        if version is not None and version >= 3:
            e["version"] = version
        journal.append(e)
        kept[c.index] = e

    for c in todo:
        try:
            fut = tracer(c.sample_offset, c.n_samples, c.file + ".partial")
        except BaseException:
            # chunks already handed to the tracer still complete: journal those whose files do
            # before the failure propagates (a resume then re-traces only what was lost)
            for pc, pf in pending:
                try:
                    finish(pc, pf)
                except Exception:  # noqa: BLE001 - the original failure is the one to report
                    break
            raise
        pending.append((c, fut))
        # journal entries are appended in chunk order, as soon as each file is complete
        while pending and (len(pending) > 1 or pending[0][1].done()):
            finish(*pending.pop(0))
    while pending:
        finish(*pending.pop(0))
    return [shard.ShardEntry(rank, c.sample_offset, c.n_samples, kept[c.index]["digest"], kept[c.index]["file"])
            for c in chunks]


class GraphModuleTracer:
    """Device tracer over built GraphModules (one per distinct chunk size): chunk c's pinned
    image is written to its file by a writer thread while chunk c+1 runs on the GPU.

    With ``packed`` the files are packed trace files: the runs are compute-only, and two packers
    (a device wire buffer and a pinned staging each) alternate, so chunk c's copy and file write
    overlap chunk c+1's kernels; the record buffers are free as soon as the pack call returns.
    With ``bias`` as well the files are version 3 (PackedCapture(bias=True))."""

    def __init__(self, build_module: Callable[[int], "object"], inputs: Callable[[int, int], "object"],
                 model: str = "graph", input_name: str = "data", rank: int = 0, world: int = 1,
                 packed: bool = False, stats: bool = False, bias: bool = False):
        if bias and not packed:
            raise ValueError("GraphModuleTracer: bias coding is a coding of packed files (packed=True)")
        self.build_module = build_module
        self.inputs = inputs
        self.model, self.input_name, self.rank, self.world = model, input_name, rank, world
        self.packed = bool(packed)
        self.bias = bool(bias)
        self.file_version = tf.PACKED_BIAS_VERSION if self.bias else tf.PACKED_VERSION if self.packed else tf.TRACE_VERSION
        # with ``stats`` every chunk's per-record statistics are reduced on the device right after
        # its run and written beside the chunk file as <chunk file>.stats.json (stats_file)
        self.record_stats = bool(stats)
        self.accumulators: Dict[int, "object"] = {}  # n_samples -> the module's StatsAccumulator
        self.stats_slots: Dict[int, "object"] = {}  # per trace image: pinned host copy of its statistics
        self.stats: List[dict] = []  # packed: per chunk {"pack_ms", "copy_ms", "write_ms", "bytes"}
        self.modules: Dict[int, list] = {}  # n_samples -> [GraphModule, [TraceCapture x2], next slot]
        self.writer = concurrent.futures.ThreadPoolExecutor(max_workers=1)
        self.busy: Dict[int, "concurrent.futures.Future"] = {}
        self.digest_slots: Dict[int, "object"] = {}  # per trace image: pinned host copy of its digest

    def _module(self, n: int, captures: bool = True):
        if n not in self.modules:
            m = self.build_module(n)
            # traced runs as one replayed HIP graph: one host call per chunk, so a host that issues
            # calls late cannot starve the copies (profiles/r03r_run_modes_slow_host.txt)
            m.module.use_graph = True
            self.modules[n] = [m, None, 0]
        entry = self.modules[n]
        if captures and entry[1] is None:  # a tracer that only checks files needs no trace images
            from .contrib.graph_executor import PackedCapture, TraceCapture
            m = entry[0]
            entry[1] = ([m.packed_capture(self.bias), PackedCapture(m.module, m._meta, bias=self.bias)] if self.packed else
                        [m.trace_capture(), TraceCapture(m.module, m._meta)])
        return entry

    def __call__(self, sample_offset: int, n_samples: int, path: str):
        import torch
        entry = self._module(n_samples)
        m, caps, slot = entry
        cap = caps[slot]
        entry[2] = 1 - slot
        prev = self.busy.get(id(cap))
        if prev is not None:
            prev.result()  # the writer is done with this image
        meta = dict(model=self.model, sample_offset=sample_offset, n_samples=n_samples, rank=self.rank,
                    world=self.world)
        m._meta.update(meta)
        cap.update_meta(**meta)
        m.set_input(self.input_name, self.inputs(sample_offset, n_samples))
        stream = torch.cuda.current_stream(m.module.device)
        if self.packed:
            m.module.run(stream)
        else:
            cap.capture_inputs(stream)
            m.module.run(stream, cap.capture_stream, cap.host_dst)
        # device digest of exactly these records, copied on the stream into this image's own
        # pinned slot: the module's digest tensor is reused by the next chunk's run, which the
        # stream may reach before the writer thread reads the value
        digest = m.module.records_digest(stream)
        slot_t = self.digest_slots.get(id(cap))
        if slot_t is None:
            slot_t = self.digest_slots[id(cap)] = torch.empty(digest.shape, dtype=digest.dtype, pin_memory=True)
        slot_t.copy_(digest, non_blocking=True)
        acc = stats_t = None
        if self.record_stats:
            # the statistics of exactly these records, on the run's stream before the next run can
            # overwrite the buffers; like the digest they go into this image's own pinned slot,
            # since the accumulator's entries are reset for the next chunk
            acc = self.accumulator(n_samples)
            acc.reset(stream)
            acc.add(stream)
            stats_t = self.stats_slots.get(id(cap))
            if stats_t is None:
                stats_t = self.stats_slots[id(cap)] = torch.empty(acc.words, dtype=torch.int64, pin_memory=True)
            acc.copy_to(stats_t, stream)
        if self.packed:
            cap.pack(stream)  # waits for the run; the copy into the staging is on the packer's stream
        done = torch.cuda.Event()
        done.record(stream)

        def write() -> int:
            done.synchronize()
            cap.synchronize()
            cap.write(path)
            if self.packed:
                self.stats.append(dict(cap.stats, bytes=cap.size))
            if acc is not None:
                final = path[:-len(".partial")] if path.endswith(".partial") else path
                write_stats_file(stats_file(final), acc.decode(stats_t))
            return int(slot_t.reshape(-1)[0].item()) & 0xFFFFFFFFFFFFFFFF

        fut = self.writer.submit(write)
        self.busy[id(cap)] = fut
        return fut

    def accumulator(self, n_samples: int):
        """The statistics accumulator of the module of ``n_samples`` (one per module)."""
        if n_samples not in self.accumulators:
            self.accumulators[n_samples] = self._module(n_samples, captures=False)[0].stats_accumulator()
        return self.accumulators[n_samples]

    def stats_only(self, sample_offset: int, n_samples: int) -> None:
        """One chunk, compute only, merged into its module's accumulator: nothing is copied or
        waited for."""
        import torch
        m = self._module(n_samples, captures=False)[0]
        acc = self.accumulator(n_samples)
        m.set_input(self.input_name, self.inputs(sample_offset, n_samples))
        stream = torch.cuda.current_stream(m.module.device)
        m.module.run(stream)
        acc.add(stream)

    def check(self, path: str, replay: bool = False):
        """Verify one chunk file, packed or not, on the device (GraphModule.verify_trace; with
        ``replay`` GraphModule.replay_trace: every op from its recorded inputs): the module is the
        one of the file's own ``n_samples``, and each module keeps one verifier.  Returns the
        VerifyReport / ReplayReport; ValueError for a file that does not parse or is of another graph."""
        with open(path, "rb") as f:
            head = f.read(56)
            jl = tf._header(head)[1]
            try:
                n = int(json.loads(f.read(jl).decode())["n_samples"])
            except (ValueError, KeyError, TypeError):
                raise ValueError(f"{path}: the trace header does not state n_samples") from None
        if not 1 <= n <= 1 << 20:
            raise ValueError(f"{path}: n_samples {n}")
        m = self._module(n, captures=False)[0]
        return m.replay_trace(path) if replay else m.verify_trace(path)

    def close(self) -> None:
        """Wait for the writer, then release every module (device first, then the native module:
        GraphModule.close) while the HIP runtime is alive."""
        self.writer.shutdown(wait=True)
        for m, caps, _ in self.modules.values():
            m.close()
            if caps is not None:
                caps.clear()
        self.modules.clear()
        self.digest_slots.clear()
        self.accumulators.clear()
        self.stats_slots.clear()


def check(tracer: GraphModuleTracer, out_dir: str, rank: int = 0, stem: str = "trace",
          log: Optional[Callable[[str], None]] = None, replay: bool = False) -> List[dict]:
    """Verify every journalled chunk file of this rank against the engine, in chunk order, following
    each file's own version: one dict per chunk, {"chunk", "file", "ok", "n_mismatched", "first":
    {name, op, first_index} | None, "params_equal", **stats}.  A missing or unreadable file, or one
    that does not parse or is of another graph, is ``ok: False`` with ``"error"``.  With ``replay``
    each chunk is replayed op by op from its recorded inputs instead (GraphModule.replay_trace) and
    the dict also has "nodes": [{node, kind, records, first}] of the faulty nodes and "ops": [{name,
    op, node, place, basis, count, first_index}] of the faulty ops (ReplayReport.ops)."""
    out = []
    for index, e in sorted(Journal(journal_file(out_dir, rank, stem)).entries().items()):
        row = {"chunk": index, "file": e.get("file")}
        try:
            path = os.path.join(out_dir, str(e.get("file")))
            rep = tracer.check(path, replay=True) if replay else tracer.check(path)
        except (OSError, ValueError) as err:
            row.update(ok=False, error=f"{type(err).__name__}: {err}")
        else:
            f = rep.first
            row.update(ok=rep.ok, n_mismatched=len(rep.mismatches),
                       first=None if f is None else {"name": f.name, "op": f.op, "first_index": list(f.first_index)},
                       params_equal=rep.params_equal, **rep.stats)
            if replay:
                row["nodes"] = [{"node": n.node, "kind": n.kind, "records": list(n.records), "first": n.first}
                                for n in rep.nodes]
                row["ops"] = [{"name": o.name, "op": o.op, "node": o.node, "place": o.place, "basis": o.basis,
                               "count": o.count, "first_index": list(o.first_index)} for o in rep.ops]
        if log:
            log(f"rank {rank}: chunk {index} {'ok' if row['ok'] else 'FAILED'}")
        out.append(row)
    return out


def stats_file(chunk_path: str) -> str:
    """The statistics sidecar of a chunk file."""
    return chunk_path + ".stats.json"


def rank_stats_file(out_dir: str, rank: int, stem: str = "trace") -> str:
    return os.path.join(out_dir, f"{stem}.rank{rank}.stats.json")


def write_stats_file(path: str, stats: Dict[str, "tf.RecordStats"]) -> None:
    """{name: RecordStats.to_json()} as one JSON object, written under a temporary name and renamed:
    a reader sees the whole file or none."""
    tmp = path + ".tmp"
    with open(tmp, "w") as f:
        json.dump(tf.stats_to_json(stats), f, separators=(",", ":"))
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def read_stats_file(path: str) -> Dict[str, "tf.RecordStats"]:
    with open(path) as f:
        return tf.stats_from_json(json.load(f))


def merge_stats(out_dir: str, rank: int = 0, stem: str = "trace",
                log: Optional[Callable[[str], None]] = None) -> Dict[str, "tf.RecordStats"]:
    """Merge the statistics of every journalled chunk of this rank, in chunk order, into
    ``<stem>.rank<r>.stats.json`` and return them.  A chunk's statistics come from its sidecar
    (stats_file); where that is missing or does not parse they are recomputed on the host from the
    chunk file itself (trace_format.trace_stats), which the log says."""
    parts = []
    for index, e in sorted(Journal(journal_file(out_dir, rank, stem)).entries().items()):
        path = os.path.join(out_dir, str(e.get("file")))
        try:
            parts.append(read_stats_file(stats_file(path)))
        except (OSError, ValueError, KeyError, TypeError):
            if log:
                log(f"rank {rank}: chunk {index} has no statistics file, reducing {os.path.basename(path)} on the host")
            parts.append(tf.trace_stats(path))
    merged = tf.merge_stats_dicts(parts)
    write_stats_file(rank_stats_file(out_dir, rank, stem), merged)
    return merged


def run_stats_only(tracer: GraphModuleTracer, global_samples: int, chunk: int, out_dir: str, rank: int = 0,
                   world: int = 1, stem: str = "trace",
                   log: Optional[Callable[[str], None]] = None) -> Dict[str, "tf.RecordStats"]:
    """The statistics of this rank's samples without a trace: every chunk runs compute-only and is
    merged on the device (one statistics launch per chunk, no record leaves the device); at the end
    the accumulators are read and ``<stem>.rank<r>.stats.json`` is written.  No chunk file and no
    journal: the job is not resumable."""
    os.makedirs(out_dir, exist_ok=True)
    chunks = plan_chunks(global_samples, world, rank, chunk, out_dir, stem)
    if log:
        log(f"rank {rank}: {len(chunks)} chunks, statistics only")
    for c in chunks:
        tracer.stats_only(c.sample_offset, c.n_samples)
    merged = tf.merge_stats_dicts([tracer.accumulators[n].result() for n in sorted(tracer.accumulators, reverse=True)])
    write_stats_file(rank_stats_file(out_dir, rank, stem), merged)
    return merged


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model", default="resnet50")
    p.add_argument("--samples", type=int, required=True, help="global number of samples")
    p.add_argument("--chunk", type=int, default=64, help="samples per chunk (one traced batch)")
    p.add_argument("--out-dir", required=True)
    p.add_argument("--no-resume", action="store_true", help="start over (drop the journal)")
    p.add_argument("--verify", action="store_true", help="re-digest resumed chunk files")
    p.add_argument("--packed", action="store_true",
                   help="write packed (version 2) chunk files: the wire coding on disk, expanded on read")
    p.add_argument("--bias-coding", action="store_true",
                   help="with --packed: write version-3 chunk files, whose bias_add records are coded as the record "
                        "before them plus the bias, stored in the file")
    p.add_argument("--check", action="store_true",
                   help="trace nothing: verify every journalled chunk file against the engine, record by record, "
                        "on the device; one JSON line per chunk, exit status 1 if any chunk fails")
    p.add_argument("--replay", action="store_true",
                   help="with --check: replay every chunk op by op from its recorded inputs instead, so that a "
                        "fault stays in its node; the JSON line also lists the faulty nodes")
    p.add_argument("--stats", action="store_true",
                   help="reduce every chunk's records to per-record statistics on the device and write them beside "
                        "the chunk file (<chunk file>.stats.json); at the end merge them into "
                        "<stem>.rank<r>.stats.json")
    p.add_argument("--stats-only", action="store_true",
                   help="write no chunk files and no journal: run the chunks compute-only, accumulate the statistics "
                        "on the device and write <stem>.rank<r>.stats.json at the end; not resumable")
    args = p.parse_args(argv)
    if args.replay and not args.check:
        p.error("--replay goes with --check")
    if args.bias_coding and not args.packed:
        p.error("--bias-coding goes with --packed")
    if args.stats_only and (args.check or args.stats or args.packed or args.verify):
        p.error("--stats-only writes no trace: it does not go with --check, --stats, --packed or --verify")
    import torch
    from . import relay, zoo
    from .contrib import graph_executor
    rank, world, local = shard.dist_env()
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo")  # manifest exchange only; no data-path collective
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    model_fn = zoo.MODELS[args.model]
    proto = model_fn(batch=1)

    def build_module(n: int):
        mdl = model_fn(batch=n)
        lib = relay.build(mdl.mod, target="mi355x", params=mdl.params)
        return graph_executor.GraphModule(lib["default"](device.index))

    tracer = GraphModuleTracer(build_module, proto.sample_inputs, model=proto.name, input_name=proto.input_name,
                               rank=rank, world=world, packed=args.packed, stats=args.stats, bias=args.bias_coding)
    log = lambda s: print(f"[trace_job] {s}", file=sys.stderr, flush=True)  # noqa: E731
    if args.stats_only:
        try:
            run_stats_only(tracer, args.samples, args.chunk, args.out_dir, rank, world, log=log)
        finally:
            tracer.close()
            if world > 1:
                import torch.distributed as dist
                dist.destroy_process_group()
        log(f"statistics {rank_stats_file(args.out_dir, rank)}")
        return 0
    if args.check:
        try:
            rows = check(tracer, args.out_dir, rank, log=log, replay=args.replay)
        finally:
            tracer.close()
            if world > 1:
                import torch.distributed as dist
                dist.destroy_process_group()
        for row in rows:
            print(json.dumps(dict(row, rank=rank)), flush=True)
        return 0 if rows and all(r["ok"] for r in rows) else 1
    try:
        entries = run(tracer, args.samples, args.chunk, args.out_dir, rank, world, resume=not args.no_resume,
                      verify=args.verify, log=log, packed=args.packed)
    finally:
        tracer.close()
    if args.stats:
        merge_stats(args.out_dir, rank, log=log)
        log(f"statistics {rank_stats_file(args.out_dir, rank)}")
    if world > 1:
        import torch.distributed as dist
        allents: List = [None] * world
        dist.all_gather_object(allents, entries)
        entries = [e for es in allents for e in es]
        dist.destroy_process_group()
    if rank == 0:
        path = os.path.join(args.out_dir, "trace.manifest.json")
        shard.write_manifest(path, proto.name, args.samples, entries, world=world)
        log(f"manifest {path}: {len(entries)} chunks")
    return 0


if __name__ == "__main__":
    sys.exit(main())
