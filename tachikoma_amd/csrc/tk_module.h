// tk_module, the native node executor's state, as its two sources see it: tk_runtime.cc (nodes,
// per-node copies, whole-run graphs, chain check, tuner) and tk_capture.cc (the packed capture).
#pragma once

#include <atomic>
#include <memory>
#include <utility>
#include <vector>

#include "tk_node.h"
#include "tk_ops.h"

namespace tk {

// A move-only HIP handle or allocation, released with `Destroy` unless it is null.
template <typename T, auto Destroy>
struct Owned {
  T h{};
  Owned() = default;
  Owned(Owned&& o) noexcept : h(std::exchange(o.h, T{})) {}
  Owned& operator=(Owned&& o) noexcept {
    std::swap(h, o.h);
    return *this;
  }
  ~Owned() {
    if (h) (void)Destroy(h);
  }
  operator T() const { return h; }
  T* put() { return &h; }  // for the call that creates it
};
using OwnedEvent = Owned<hipEvent_t, hipEventDestroy>;
using OwnedStream = Owned<hipStream_t, hipStreamDestroy>;
using OwnedGraph = Owned<hipGraph_t, hipGraphDestroy>;
using OwnedGraphExec = Owned<hipGraphExec_t, hipGraphExecDestroy>;
template <typename T>
using OwnedDev = Owned<T*, hipFree>;
using OwnedPinned = Owned<void*, hipHostFree>;

// run_packed's "nothing to capture, run the plain graph" answer (not an error code)
constexpr int TK_OK_RUN = 1;

int run_node(Node& n, hipStream_t s);

// one captured whole-run graph of a module (tk_module::graphs)
struct RunGraph {
  OwnedGraph g;
  OwnedGraphExec ge;
  hipStream_t s = nullptr, cs = nullptr;
  std::vector<void*> dst;
};

}  // namespace tk

struct PackPlan;  // tk_capture.cc
struct PackPlanDelete {
  void operator()(PackPlan* p) const;
};

struct tk_module {
  std::vector<tk::Node> nodes;
  // Streams of the module's own come first, so that they are released after the events below.
  // The graphs are captured on cap_s / cap_cs / cap_cx (the caller's may be the legacy default
  // stream, which cannot capture) and launched on the caller's; wire traffic and decodes of the
  // packed capture run on wire_s / dec_s.
  tk::OwnedStream cap_s, cap_cs, cap_cx[3], wire_s, dec_s;
  std::vector<tk::OwnedEvent> done;  // one per node, recorded after it on the compute stream
  std::vector<tk::OwnedEvent> prof;  // n+1 timing events for run_profiled / profiling mode
  // Recorded on the capture stream after the last D2H copy of a traced run.  Every later
  // run (and, through tk_module_wait_capture, every input write) first makes its stream wait
  // on it: the copies read the module's buffers, so overwriting them before the copies land
  // would mix two runs in one trace image (write-after-read across streams).
  tk::OwnedEvent capture_done;
  bool capture_recorded = false;
  bool capture_plain = false;  // the last capture copied from the record buffers themselves
  bool profiling = false;
  bool have_times = false;
  // tk_module_run_graph: the whole run (every node, and the copies when capturing) as one HIP
  // graph per (stream, capture stream, host destinations), instantiated once and replayed; a few
  // are kept (a file sink alternates two trace images)
  std::vector<tk::RunGraph> graphs;
  tk::OwnedEvent graph_join, graph_pre;
  // graph copies as copy kernels instead of memcpy nodes: measured slower (41.7 vs 52.7 GB/s per
  // traced ResNet-50 step, profiles/r03n_run_modes.txt), so off by default
  bool graph_copy_kernels = false;
  // memcpy nodes in this many parallel chains (1..4): 4 measured 53.4 GB/s per traced ResNet-50
  // step against 52.7 for one chain (profiles/r03s_graph_copy_chains.txt)
  int graph_copy_chains = 4;
  // packed capture (default): records gathered into device mirrors, copied in this many chunks
  bool graph_packed = true;
  int pack_chunks = 8;
  std::vector<std::unique_ptr<PackPlan, PackPlanDelete>> packs;
  // copy trace of packed runs (tk_module_set_copy_trace): a timing event on the compute stream
  // before the run's first launch, and two per chunk on the capture stream around its copy
  bool copy_trace = false;
  tk::OwnedEvent ct_t0;
  std::vector<tk::OwnedEvent> ct_ev;
  std::vector<int64_t> ct_bytes;
  // trace wire of the packed capture: on unless TK_TRACE_WIRE=0 was set when the module was created
  // TK_WIRE_CLAMP=0 at creation keeps the clip records raw (the same library's comparison run)
  // TK_WIRE_BIAS=0 at creation keeps the bias_add records plain differences (likewise)
  bool trace_wire = true, wire_forced_off = false, wire_clamp = true, wire_bias = true;
  tk::OwnedEvent wire_tail, decode_tail;  // last wire work / decode of the last wire run
  bool wire_tail_used = false;
  std::atomic<int> wire_failed{0};
  PackPlan* last_wire_plan = nullptr;
  // chain check (tk_module_check_chains): the table of the module's fused chains, laid out on the
  // first call and kept on the device with its report, so later calls upload nothing
  struct Chains {
    bool built = false;
    std::vector<tk_chain_op> ops;  // one per report entry: node order, then chain order
    int n_chains = 0;
    int64_t blocks = 0;
    tk::OwnedDev<void> dev;  // ChainDev[n_chains] | tk_wire_mismatch[ops.size()]
    tk_wire_mismatch* report = nullptr;
  } chains;
  void drop_graph() {
    last_wire_plan = nullptr;
    graphs.clear();
    if (!packs.empty()) (void)hipDeviceSynchronize();  // their mirrors may still be copied from
    packs.clear();
  }
  ~tk_module() { drop_graph(); }
};

namespace tk {

// The stream about to write the module's buffers waits for the last traced run's copies.
inline int wait_capture(tk_module* mod, hipStream_t s) {
  if (mod->capture_recorded) TK_HIP(hipStreamWaitEvent(s, mod->capture_done, 0));
  return TK_OK;
}

// One packed traced run (tk_capture.cc); TK_OK_RUN: no record has a host destination.
int run_packed(tk_module* mod, hipStream_t s, hipStream_t cs, void* const* host_dst);

}  // namespace tk
