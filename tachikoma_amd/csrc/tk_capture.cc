// Packed trace capture for tk_module_run_graph (the default graph copy mode): the node outputs that
// have host destinations are gathered, chunk by chunk, into a device mirror of the host image range
// they span (header bytes included, loaded once from the host image), and each chunk is copied to
// host memory by ONE host-issued hipMemcpyAsync gated on an event recorded after the graph that
// ends with the chunk's pack kernel (one graph per chunk).  Two mirrors alternate between runs, so a run's kernels overlap the previous
// run's copies (only the pack into a mirror waits for that mirror's last copies).
//
// What is captured how is planned without HIP by tk_capture_plan.cc; this file gives the plan its
// device and pinned memory, graphs, streams and events, and runs it.
#include <algorithm>
#include <atomic>
#include <memory>
#include <string>
#include <vector>

#include "tk_capture_plan.h"
#include "tk_module.h"

struct PackPlan : tk::CapturePlan {
  std::vector<void*> dst;         // host_dst this plan was built for (the cache key)
  tk::OwnedDev<char> mirror[2];
  tk::OwnedDev<tk::PackRec> dev_table;    // `table` on the device
  std::vector<tk::OwnedEvent> ev[2];      // per chunk, recorded after its graph
  tk::OwnedEvent mirror_done[2];
  bool mirror_used[2] = {false, false};
  std::vector<tk::OwnedGraph> g[2];       // per mirror: one graph per chunk (+ a tail graph)
  std::vector<tk::OwnedGraphExec> ge[2];
  int next = 0;
  // Trace wire (tk_module_set_trace_wire): what a chunk's wire work needs besides its WireChunk
  struct WireCall {  // what one decode host function works on
    tk::WireJob job;
    std::atomic<int>* failed = nullptr;
  };
  struct WireRun {
    std::unique_ptr<WireCall[]> calls;  // one per slot
    tk::OwnedEvent landed;              // the chunk's wire work is done
    int last_slot = -1;
  };
  std::vector<WireRun> wrun;              // one per chunk where `wire`
  tk::OwnedDev<tk::WireSegDev> dev_segs;  // `wire_segs` on the device
  // Bias coding: the bias vectors of the records coded with an addend, copied once when the plan
  // is built.  The encoder subtracts the device copy and the decoder adds the host copy, which is
  // a copy of that device copy; neither reads a node's live bias, so new parameters can make the
  // prediction worse but never the two sides disagree.
  tk::OwnedDev<int32_t> addend_dev;
  std::vector<int32_t> addend_host;
  std::vector<tk::OwnedPinned> slots;     // pinned ring of worst-case-sized chunk slots
  tk::OwnedDev<uint32_t> cursors;         // device, one per slot
  std::vector<tk::OwnedEvent> slot_done;  // decode of the slot's last use (decode stream)
  std::vector<char> slot_used;
  int slot_next = 0;
};

void PackPlanDelete::operator()(PackPlan* p) const { delete p; }

namespace tk {

// The plan's snapshot of the bias vectors its records are coded with (PackPlan::addend_dev /
// addend_host): each vector copied device to device into one buffer, and that buffer to the host.
static int snapshot_addends(PackPlan* plan) {
  const int64_t total = plan->addend_total;
  if (!total) return TK_OK;
  TK_HIP(hipMalloc(plan->addend_dev.put(), (size_t)total * sizeof(int32_t)));
  for (const CaptureRecord& r : plan->recs)
    if (r.bias)
      TK_HIP(hipMemcpy(plan->addend_dev + r.addend_at, ptr(r.bias), (size_t)r.channels * sizeof(int32_t),
                       hipMemcpyDeviceToDevice));
  plan->addend_host.resize((size_t)total);
  TK_HIP(hipMemcpy(plan->addend_host.data(), plan->addend_dev, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost));
  return TK_OK;
}

// The device pack table, two mirrors and their events; on the wire also the device segment table,
// a ring of pinned slots each large enough for any chunk with every block raw, a cursor per slot,
// the decode calls of every (chunk, slot) pair and the module's streams.
static int alloc_pack_resources(tk_module* mod, PackPlan* plan) {
  const std::vector<PackRec>& table = plan->table;
  if (!table.empty()) {
    TK_HIP(hipMalloc(plan->dev_table.put(), table.size() * sizeof(PackRec)));
    TK_HIP(hipMemcpy(plan->dev_table, table.data(), table.size() * sizeof(PackRec), hipMemcpyHostToDevice));
  }
  if (plan->wire) {
    const std::vector<WireSegDev>& wire_segs = plan->wire_segs;
    TK_HIP(hipMalloc(plan->dev_segs.put(), wire_segs.size() * sizeof(WireSegDev)));
    TK_HIP(hipMemcpy(plan->dev_segs, wire_segs.data(), wire_segs.size() * sizeof(WireSegDev), hipMemcpyHostToDevice));
    int64_t slot_bytes = 0;
    int coded_chunks = 0;
    for (const auto& w : plan->wchunks) slot_bytes = std::max(slot_bytes, w.bound), coded_chunks += !w.segs.empty();
    const int n_slots = std::min(3, coded_chunks);
    for (int k = 0; k < n_slots; ++k) {
      OwnedPinned p;
      TK_HIP(hipHostMalloc(p.put(), (size_t)slot_bytes, hipHostMallocDefault));
      plan->slots.push_back(std::move(p));
      OwnedEvent e;
      TK_HIP(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
      plan->slot_done.push_back(std::move(e));
    }
    plan->slot_used.assign(n_slots, 0);
    TK_HIP(hipMalloc(plan->cursors.put(), n_slots * sizeof(uint32_t)));
    plan->wrun.resize(plan->wchunks.size());
    for (size_t c = 0; c < plan->wchunks.size(); ++c) {
      const CapturePlan::WireChunk& w = plan->wchunks[c];
      if (w.segs.empty()) continue;
      PackPlan::WireRun& wr = plan->wrun[c];
      TK_HIP(hipEventCreateWithFlags(wr.landed.put(), hipEventDisableTiming));
      wr.calls.reset(new PackPlan::WireCall[n_slots]);
      for (int k = 0; k < n_slots; ++k) {
        WireJob& j = wr.calls[k].job;
        j.wire = (const char*)plan->slots[k].h;
        j.wire_bytes = w.bound;
        j.segs = w.segs.data(), j.n_seg = (int64_t)w.segs.size();
        j.units = w.units.data(), j.n_units = (int64_t)w.units.size();
        wr.calls[k].failed = &mod->wire_failed;
      }
    }
    if (!mod->wire_s) TK_HIP(hipStreamCreateWithFlags(mod->wire_s.put(), hipStreamNonBlocking));
    if (!mod->dec_s) TK_HIP(hipStreamCreateWithFlags(mod->dec_s.put(), hipStreamNonBlocking));
    if (!mod->wire_tail) TK_HIP(hipEventCreateWithFlags(mod->wire_tail.put(), hipEventDisableTiming));
    if (!mod->decode_tail) TK_HIP(hipEventCreateWithFlags(mod->decode_tail.put(), hipEventDisableTiming));
  }
  for (int m = 0; m < 2; ++m) {
    // the mirror holds the image's bytes between records (headers) from the start
    TK_HIP(hipMalloc(plan->mirror[m].put(), (size_t)plan->span + 16));
    TK_HIP(hipMemcpy(plan->mirror[m], plan->host_lo, (size_t)plan->span, hipMemcpyHostToDevice));
    TK_HIP(hipEventCreateWithFlags(plan->mirror_done[m].put(), hipEventDisableTiming));
    for (size_t c = 0; c < plan->chunks.size(); ++c) {
      OwnedEvent e;
      TK_HIP(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
      plan->ev[m].push_back(std::move(e));
    }
  }
  if (!mod->cap_s) TK_HIP(hipStreamCreateWithFlags(mod->cap_s.put(), hipStreamNonBlocking));
  return TK_OK;
}

// One graph per chunk and mirror: the nodes up to the chunk's last producer and its pack kernel (a
// tail graph holds the nodes after the last chunk).  The copy of chunk c waits on an event recorded
// between graph launches c and c + 1; external event-record nodes inside one graph would do the
// same in one launch, but torch's bundled HIP runtime (7.0) refuses them in capture.
static int capture_chunk_graphs(tk_module* mod, PackPlan* plan) {
  const int nn = (int)mod->nodes.size();
  const int nseg = (int)plan->chunks.size() + (plan->chunks.back().after_node < nn - 1 ? 1 : 0);
  for (int m = 0; m < 2; ++m) {
    hipStream_t qs = mod->cap_s;
    int i = 0;
    for (int seg = 0; seg < nseg; ++seg) {
      const bool has_chunk = seg < (int)plan->chunks.size();
      const int last = has_chunk ? plan->chunks[seg].after_node : nn - 1;
      TK_HIP(hipStreamBeginCapture(qs, hipStreamCaptureModeThreadLocal));
      int rc = TK_OK;
      for (; i <= last && rc == TK_OK; ++i) {
        rc = run_node(mod->nodes[i], qs);
        if (rc) set_error("node " + std::to_string(i) + ": " + tk_last_error());
      }
      if (rc == TK_OK && has_chunk && plan->chunks[seg].n_rec > 0) {
        const CapturePlan::Chunk& ch = plan->chunks[seg];
        rc = pack_records_impl(plan->dev_table + ch.table_off, ch.n_rec, ch.blocks, plan->mirror[m], qs);
      }
      OwnedGraph g;
      hipError_t e = hipStreamEndCapture(qs, g.put());
      if (rc) return rc;
      if (e != hipSuccess || !g) {
        (void)hipGetLastError();
        set_error(std::string("tk_module_run_graph: stream capture failed: ") + hipGetErrorString(e));
        return TK_ERR_HIP;
      }
      plan->g[m].push_back(std::move(g));
      OwnedGraphExec ge;
      e = hipGraphInstantiate(ge.put(), plan->g[m].back(), nullptr, nullptr, 0);
      if (e != hipSuccess) {
        set_error(std::string("tk_module_run_graph: instantiate failed: ") + hipGetErrorString(e));
        return TK_ERR_HIP;
      }
      plan->ge[m].push_back(std::move(ge));
    }
  }
  return TK_OK;
}

// Builds the packed-capture plan for host destinations `dst`: the mirrored range, the chunks (cut
// at node boundaries where every record below the cut is written), the device pack tables, two
// mirrors loaded with the host image's bytes, and one graph per chunk and mirror.
static int build_pack_plan(tk_module* mod, const std::vector<void*>& dst, PackPlan** out) {
  std::unique_ptr<PackPlan, PackPlanDelete> plan(new PackPlan);
  plan->dst = dst;
  const CaptureOptions opt{mod->pack_chunks, mod->trace_wire && !mod->wire_forced_off, mod->wire_clamp, mod->wire_bias};
  if (const int rc = capture_plan_records(mod->nodes, dst.data(), opt, plan.get())) return rc;
  if (plan->recs.empty()) {
    *out = nullptr;
    return TK_OK;
  }
  // first, so that the segments are planned with the snapshot's final addresses
  if (const int rc = snapshot_addends(plan.get())) return rc;
  if (const int rc = capture_plan_chunks((int)mod->nodes.size(), opt.chunks, plan->addend_dev, plan->addend_host.data(),
                                         plan.get()))
    return rc;
  if (const int rc = alloc_pack_resources(mod, plan.get())) return rc;
  if (const int rc = capture_chunk_graphs(mod, plan.get())) return rc;
  *out = plan.release();
  return TK_OK;
}

// The decode host function of one chunk (decode stream): widens the chunk's slot into the image
// on the decoder's pool and waits for it; no HIP call.
static void wire_decode_call(void* p) {
  auto* call = static_cast<PackPlan::WireCall*>(p);
  if (wire_decode(&call->job, 0)) call->failed->store(1);
}

// The wire side of one chunk of a packed run, after the chunk's graph and its event on s:
//   s       graph c | ev ................ graph c+1 | ev ...
//   wire_s  wait ev, wait slot_done[k] | cursor = 0 | encode -> slot k | raw copies | landed[c]
//   dec_s   wait landed[c] | host function: decode slot k -> image | slot_done[k]
static int enqueue_wire_chunk(tk_module* mod, PackPlan* plan, int m, size_t c, bool trace) {
  const CapturePlan::Chunk& ch = plan->chunks[c];
  const CapturePlan::WireChunk& w = plan->wchunks[c];
  PackPlan::WireRun& wr = plan->wrun[c];
  hipStream_t ws = mod->wire_s, ds = mod->dec_s;
  TK_HIP(hipStreamWaitEvent(ws, plan->ev[m][c], 0));
  if (trace) TK_HIP(hipEventRecord(mod->ct_ev[2 * c], ws));
  int k = -1;
  if (!w.segs.empty()) {
    k = plan->slot_next;
    plan->slot_next = (k + 1) % (int)plan->slots.size();
    if (plan->slot_used[k]) TK_HIP(hipStreamWaitEvent(ws, plan->slot_done[k], 0));
    TK_HIP(hipMemsetAsync(plan->cursors + k, 0, sizeof(uint32_t), ws));
    const int rc = wire_encode_impl(plan->dev_segs + w.seg_off, (int64_t)w.segs.size(), plan->cursors + k,
                                    plan->slots[k], w.bound, ws);
    if (rc) return rc;
  }
  for (const CapturePlan::Range& r : w.raw)
    TK_HIP(hipMemcpyAsync(plan->host_lo + r.off, plan->mirror[m] + r.off, (size_t)r.len, hipMemcpyDeviceToHost, ws));
  if (trace) {
    TK_HIP(hipEventRecord(mod->ct_ev[2 * c + 1], ws));
    mod->ct_bytes[c] = ch.len;
  }
  if (k >= 0) {
    TK_HIP(hipEventRecord(wr.landed, ws));
    TK_HIP(hipStreamWaitEvent(ds, wr.landed, 0));
    TK_HIP(hipLaunchHostFunc(ds, wire_decode_call, &wr.calls[k]));
    TK_HIP(hipEventRecord(plan->slot_done[k], ds));
    plan->slot_used[k] = 1;
    wr.last_slot = k;
  }
  return TK_OK;
}

// One packed traced run: the chunk graphs of mirror m (kernels, pack kernel) on s, each followed by
// an event, and the chunk copies on cs, each after its event (wire runs: enqueue_wire_chunk).
int run_packed(tk_module* mod, hipStream_t s, hipStream_t cs, void* const* host_dst) {
  const size_t nd = mod->nodes.size() * TK_MAX_NODE_OUTPUTS;
  std::vector<void*> dst(host_dst, host_dst + nd);
  PackPlan* plan = nullptr;
  for (auto& p : mod->packs)
    if (p->dst == dst) plan = p.get();
  if (!plan) {
    if (mod->packs.size() >= 2) {  // keep the newest (a file sink alternates two images)
      TK_HIP(hipDeviceSynchronize());
      if (mod->last_wire_plan == mod->packs.front().get()) mod->last_wire_plan = nullptr;
      mod->packs.erase(mod->packs.begin());
    }
    PackPlan* built = nullptr;
    int rc = build_pack_plan(mod, dst, &built);
    if (rc) return rc;
    if (!built) return TK_OK_RUN;  // nothing to capture
    mod->packs.emplace_back(built);
    plan = built;
  }
  // a previous per-record (unpacked) capture still reads the record buffers on cs
  if (mod->capture_recorded && mod->capture_plain) TK_HIP(hipStreamWaitEvent(s, mod->capture_done, 0));
  const int m = plan->next;
  plan->next ^= 1;
  // the pack into mirror m waits for that mirror's last copies (two runs ago); the records the
  // kernels overwrite are only read by the packs of the previous launch on the same stream
  if (plan->mirror_used[m]) TK_HIP(hipStreamWaitEvent(s, plan->mirror_done[m], 0));
  if (mod->wire_failed.load()) {
    set_error("tk_module_run_graph: a wire buffer of an earlier run did not decode");
    return TK_ERR_INVALID_ARG;
  }
  // the encode kernels of the last wire run read the record buffers this run overwrites
  if (mod->wire_tail_used) TK_HIP(hipStreamWaitEvent(s, mod->wire_tail, 0));
  const bool trace = mod->copy_trace;
  if (trace) {
    if (!mod->ct_t0) TK_HIP(hipEventCreate(mod->ct_t0.put()));
    while (mod->ct_ev.size() < 2 * plan->chunks.size()) {
      OwnedEvent e;
      TK_HIP(hipEventCreate(e.put()));
      mod->ct_ev.push_back(std::move(e));
    }
    mod->ct_bytes.assign(plan->chunks.size(), 0);
    TK_HIP(hipEventRecord(mod->ct_t0, s));
  }
  for (size_t c = 0; c < plan->ge[m].size(); ++c) {
    TK_HIP(hipGraphLaunch(plan->ge[m][c], s));
    if (c >= plan->chunks.size()) break;  // the tail graph
    const CapturePlan::Chunk& ch = plan->chunks[c];
    TK_HIP(hipEventRecord(plan->ev[m][c], s));
    if (plan->wire) {
      const int rc = enqueue_wire_chunk(mod, plan, m, c, trace);
      if (rc) return rc;
      continue;
    }
    TK_HIP(hipStreamWaitEvent(cs, plan->ev[m][c], 0));
    if (trace) TK_HIP(hipEventRecord(mod->ct_ev[2 * c], cs));
    TK_HIP(hipMemcpyAsync(plan->host_lo + ch.off, plan->mirror[m] + ch.off, (size_t)ch.len,
                          hipMemcpyDeviceToHost, cs));
    if (trace) {
      TK_HIP(hipEventRecord(mod->ct_ev[2 * c + 1], cs));
      mod->ct_bytes[c] = ch.len;
    }
  }
  if (plan->wire) {
    // the capture stream waits for the run's last wire work and last decode, so that capture_done
    // (and the capture stream's synchronisation) still means "the image is complete"
    TK_HIP(hipEventRecord(mod->wire_tail, mod->wire_s));
    TK_HIP(hipEventRecord(plan->mirror_done[m], mod->wire_s));
    TK_HIP(hipEventRecord(mod->decode_tail, mod->dec_s));
    mod->wire_tail_used = true;
    mod->last_wire_plan = plan;
    TK_HIP(hipStreamWaitEvent(cs, mod->wire_tail, 0));
    TK_HIP(hipStreamWaitEvent(cs, mod->decode_tail, 0));
  } else {
    TK_HIP(hipEventRecord(plan->mirror_done[m], cs));
    mod->last_wire_plan = nullptr;
  }
  plan->mirror_used[m] = true;
  TK_HIP(hipEventRecord(mod->capture_done, cs));
  mod->capture_recorded = true;
  mod->capture_plain = false;
  return TK_OK;
}

}  // namespace tk

extern "C" {

int tk_module_set_trace_chunks(tk_module* mod, int chunks) {
  if (!mod || chunks < 1 || chunks > 256) {
    tk::set_error("tk_module_set_trace_chunks: chunks must be 1..256");
    return TK_ERR_INVALID_ARG;
  }
  if (mod->pack_chunks != chunks) mod->drop_graph();
  mod->pack_chunks = chunks;
  return TK_OK;
}

int tk_module_set_copy_trace(tk_module* mod, int enable) {
  if (!mod) {
    tk::set_error("tk_module_set_copy_trace: null module");
    return TK_ERR_INVALID_ARG;
  }
  mod->copy_trace = enable != 0;
  mod->ct_bytes.clear();
  return TK_OK;
}

int tk_module_set_trace_wire(tk_module* mod, int enable) {
  if (!mod || (enable != 0 && enable != 1)) {
    tk::set_error("tk_module_set_trace_wire: invalid argument");
    return TK_ERR_INVALID_ARG;
  }
  if (mod->trace_wire != (enable != 0)) mod->drop_graph();
  mod->trace_wire = enable != 0;
  return TK_OK;
}

int tk_module_wire_stats(tk_module* mod, double* out, int max_chunks) {
  if (!mod || (max_chunks > 0 && !out)) {
    tk::set_error("tk_module_wire_stats: invalid argument");
    return TK_ERR_INVALID_ARG;
  }
  PackPlan* plan = mod->last_wire_plan;
  if (!plan) return 0;
  TK_HIP(hipEventSynchronize(mod->decode_tail));
  if (mod->wire_failed.load()) {
    tk::set_error("tk_module_wire_stats: a wire buffer did not decode");
    return TK_ERR_INVALID_ARG;
  }
  const int n = (int)plan->wchunks.size();
  for (int c = 0; c < n && c < max_chunks; ++c) {
    const tk::CapturePlan::WireChunk& w = plan->wchunks[c];
    const PackPlan::WireRun& wr = plan->wrun[c];
    const tk::WireJob* j = wr.last_slot >= 0 ? &wr.calls[wr.last_slot].job : nullptr;
    int64_t raw = 0;
    for (const tk::CapturePlan::Range& r : w.raw) raw += r.len;
    out[3 * c] = (double)((j ? j->used_bytes : 0) + raw);
    out[3 * c + 1] = (double)w.coded_bytes;
    out[3 * c + 2] = j ? j->ms : 0.0;
  }
  return n;
}

int tk_module_copy_trace(tk_module* mod, double* out, int max_chunks) {
  if (!mod || (max_chunks > 0 && !out)) {
    tk::set_error("tk_module_copy_trace: invalid argument");
    return TK_ERR_INVALID_ARG;
  }
  const int n = (int)mod->ct_bytes.size();
  for (int c = 0; c < n && c < max_chunks; ++c) {
    float a = 0.f, b = 0.f;
    TK_HIP(hipEventSynchronize(mod->ct_ev[2 * c + 1]));
    TK_HIP(hipEventElapsedTime(&a, mod->ct_t0, mod->ct_ev[2 * c]));
    TK_HIP(hipEventElapsedTime(&b, mod->ct_t0, mod->ct_ev[2 * c + 1]));
    out[3 * c] = (double)mod->ct_bytes[c];
    out[3 * c + 1] = a;
    out[3 * c + 2] = b;
  }
  return n;
}

}  // extern "C"
