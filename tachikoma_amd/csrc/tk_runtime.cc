// extern "C" entry points + the native node executor.
//
// tk_module is the MI355X analogue of the reference's GraphExecutor
// (src/runtime/graph_executor/graph_executor.cc:61-66 Run, :466-572 op execs)
// fused with the debug executor's per-node copy-out
// (src/runtime/graph_executor/debug/graph_executor_debug.cc:249-284): it walks a
// flat node list on one HIP stream and, when asked, copies every node output to
// host memory on a second stream, each copy gated by an event recorded right
// after the node, so the PCIe transfer of node i overlaps the kernels of nodes > i.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "tk_chain.h"
#include "tk_common.h"
#include "tk_wire.h"

namespace tk {
int requantize_impl(const tk_tensor* x, tk_tensor* y, const tk_requantize_attrs* a, hipStream_t s);
int bias_add_impl(const tk_tensor* x, const tk_tensor* b, tk_tensor* y, int axis, hipStream_t s);
int clip_impl(const tk_tensor* x, tk_tensor* y, int64_t lo, int64_t hi, hipStream_t s);
int cast_impl(const tk_tensor* x, tk_tensor* y, hipStream_t s);
int qnn_add_impl(const tk_tensor* a, const tk_tensor* b, tk_tensor* y, const tk_qnn_add_attrs* at, hipStream_t s);
int add_block_impl(const tk_tensor* a, const tk_tensor* b, tk_tensor* const* outs, int n_outs,
                   const tk_add_block_attrs* at, void* shadow, hipStream_t s);
int max_pool_impl(const tk_tensor* x, tk_tensor* y, const tk_pool2d_attrs* a, hipStream_t s);
int max_pool_shadow_impl(const tk_tensor* x, const void* x_shadow, tk_tensor* y, const tk_pool2d_attrs* a,
                         void* y_shadow, hipStream_t s);
int avg_pool_impl(const tk_tensor* x, tk_tensor* y, const tk_pool2d_attrs* a, hipStream_t s);
int global_avg_pool_impl(const tk_tensor* x, tk_tensor* y, hipStream_t s);
int copy_impl(const tk_tensor* x, tk_tensor* y, hipStream_t s);
int pad_impl(const tk_tensor* x, tk_tensor* y, const tk_pad_attrs* a, hipStream_t s);
int postops_impl(const tk_tensor* acc, const tk_tensor* sum_src, tk_tensor* y, const tk_postops_attrs* a,
                 hipStream_t s);
// tk_trace.hip: what the packed capture launches
int host_copy_impl(const void* const* src, void* const* dst, const int64_t* bytes, int n, hipStream_t s);
int pack_records_impl(const void* table, int nrec, int64_t blocks, void* mirror, hipStream_t s);
int wire_encode_impl(const WireSegDev* segs, int64_t n_seg, uint32_t* cursor, void* wire, int64_t wire_bytes,
                     hipStream_t s);
int ewise_impl(const tk_tensor* x, const tk_tensor* r, tk_tensor* y, const tk_ewise_attrs* a, hipStream_t s);
int conv2d_f32_impl(const tk_tensor* x, const tk_tensor* w, tk_tensor* y, const tk_conv2d_attrs* a, hipStream_t s);
int dense_f32_impl(const tk_tensor* x, const tk_tensor* w, tk_tensor* y, hipStream_t s);
int64_t conv_packed_weight_bytes(const tk_tensor* weight, int groups);
int conv_pack_weight(const tk_tensor* weight, int groups, void* packed, int32_t* sums, hipStream_t s);
int64_t conv_shadow_bytes(const tk_tensor* data);
int64_t conv_scratch_bytes(const tk_tensor* data, const tk_tensor* weight, const tk_conv2d_attrs* a, int block);
int make_shadow_impl(const tk_tensor* data, void* shadow, hipStream_t s);
int conv2d_prepared_impl(const tk_tensor* data, const void* shadow, const tk_tensor* weight, const void* packed,
                         const int32_t* sums, tk_tensor* out, const tk_conv2d_attrs* a, void* scratch, hipStream_t s);
int64_t conv2d_workspace_bytes(const tk_tensor* data, const tk_tensor* weight, const tk_conv2d_attrs* a);
int conv2d_impl(const tk_tensor* data, const tk_tensor* weight, tk_tensor* out, const tk_conv2d_attrs* a,
                void* workspace, hipStream_t s);
int64_t dense_workspace_bytes(const tk_tensor* data, const tk_tensor* weight);
int dense_impl(const tk_tensor* data, const tk_tensor* weight, tk_tensor* out, const tk_dense_attrs* a,
               void* workspace, hipStream_t s);
int conv2d_block_impl(const tk_tensor* data, const void* shadow, const tk_tensor* weight, const void* packed,
                      const int32_t* sums, const tk_tensor* bias, tk_tensor* const* outs, int n_outs,
                      const tk_block_attrs* attrs, void* scratch, void* shadow_out, hipStream_t s);
int dense_block_impl(const tk_tensor* data, const tk_tensor* weight, const tk_tensor* bias, tk_tensor* const* outs,
                     int n_outs, const tk_block_attrs* attrs, void* workspace, hipStream_t s);
int qnn_quantize_impl(const tk_tensor* x, tk_tensor* y, const tk_qparams_attrs* a, hipStream_t s);
int qnn_dequantize_impl(const tk_tensor* x, tk_tensor* y, const tk_qparams_attrs* a, hipStream_t s);
int qnn_binary_impl(const tk_tensor* a, const tk_tensor* b, tk_tensor* y, const tk_qnn_binary_attrs* at,
                    hipStream_t s);
int qnn_concatenate_impl(const tk_tensor* const* xs, int n_in, tk_tensor* y, const tk_concat_attrs* a,
                         hipStream_t s);
int transpose_impl(const tk_tensor* x, tk_tensor* y, const tk_transpose_attrs* a, hipStream_t s);
int conv2d_block_algos_impl(const tk_tensor* data, const tk_tensor* weight, const tk_block_attrs* attrs,
                            int32_t* algos, int max_algos);
int qnn_leaky_relu_impl(const tk_tensor* x, tk_tensor* y, const tk_leaky_relu_attrs* a, hipStream_t s);
int qnn_simulated_impl(bool quant, const tk_tensor* x, tk_tensor* y, const tk_simq_attrs* a, hipStream_t s);
int requantize_fp_impl(const tk_tensor* x, tk_tensor* y, const tk_requantize_fp_attrs* a, hipStream_t s);
int qnn_binary_fp_impl(const tk_tensor* a, const tk_tensor* b, tk_tensor* y, const tk_qnn_binary_fp_attrs* at,
                       hipStream_t s);
int qnn_lookup_impl(const tk_tensor* x, tk_tensor* y, const void* table, hipStream_t s);
int qnn_conv2d_transpose_impl(const tk_tensor* x, const tk_tensor* w, tk_tensor* y, const tk_conv2d_transpose_attrs* a,
                              hipStream_t s);

// qnn.batch_matmul (src/relay/qnn/op/batch_matmul.cc:162-228): the qnn.dense kernel per batch entry,
// on [M, K] / [N, K] / [M, N] views of x[b], y[b] (b or 0 where that operand's batch is 1), out[b];
// one workspace serves every entry (the launches are stream-ordered).
static bool bmm_check(const tk_tensor* x, const tk_tensor* y) {
  return x && y && compact(x) && compact(y) && x->ndim == 3 && y->ndim == 3 && x->shape[2] == y->shape[2] &&
         (x->shape[0] == y->shape[0] || x->shape[0] == 1 || y->shape[0] == 1);
}
struct View2 {
  int64_t shape[2];
  tk_tensor t;
  View2(const tk_tensor* src, int64_t b) {
    t = *src;
    shape[0] = src->shape[1];
    shape[1] = src->shape[2];
    t.ndim = 2;
    t.shape = shape;
    t.strides = nullptr;
    t.byte_offset = src->byte_offset + (uint64_t)(b * shape[0] * shape[1] * elem_bytes(src));
  }
};
int64_t batch_matmul_workspace_bytes(const tk_tensor* x, const tk_tensor* y) {
  if (!bmm_check(x, y)) {
    set_error("qnn.batch_matmul: x [B, M, K], y [B', N, K] with B == B' or one of them 1");
    return TK_ERR_INVALID_ARG;
  }
  View2 xv(x, 0), yv(y, 0);
  return dense_workspace_bytes(&xv.t, &yv.t);
}
int batch_matmul_impl(const tk_tensor* x, const tk_tensor* y, tk_tensor* out, const tk_dense_attrs* a, void* ws,
                      hipStream_t s) {
  TK_CHECK_ARG(bmm_check(x, y) && out && a, "qnn.batch_matmul: x [B, M, K], y [B', N, K] (B == B' or one is 1)");
  const int64_t B = std::max(x->shape[0], y->shape[0]);
  TK_CHECK_ARG(compact(out) && out->ndim == 3 && out->shape[0] == B && out->shape[1] == x->shape[1] &&
               out->shape[2] == y->shape[1] && is_int(out, 32), "qnn.batch_matmul: int32 [B, M, N] output");
  for (int64_t b = 0; b < B; ++b) {
    View2 xv(x, x->shape[0] == 1 ? 0 : b), yv(y, y->shape[0] == 1 ? 0 : b), ov(out, b);
    const int rc = dense_impl(&xv.t, &yv.t, &ov.t, a, ws, s);
    if (rc) return rc;
  }
  return TK_OK;
}
int conv2d_block_algo_info_impl(const tk_tensor* data, const tk_tensor* weight, const tk_block_attrs* attrs, int algo,
                                char* buf, int len);

// run_packed's "nothing to capture, run the plain graph" answer (not an error code)
constexpr int TK_OK_RUN = 1;

// A tensor descriptor owned by the module (shape copied).
struct OwnedTensor {
  tk_tensor t{};
  std::vector<int64_t> shape;
  void assign(const tk_tensor* src) {
    t = *src;
    shape.assign(src->shape, src->shape + src->ndim);
    t.shape = shape.data();
    t.strides = nullptr;
  }
  OwnedTensor() = default;
  OwnedTensor(const OwnedTensor& o) { assign(&o.t); }
  OwnedTensor& operator=(const OwnedTensor& o) {
    assign(&o.t);
    return *this;
  }
};

struct Node {
  tk_node desc{};
  OwnedTensor in[TK_MAX_NODE_INPUTS];
  OwnedTensor out[TK_MAX_NODE_OUTPUTS];
  tk_tensor* outp[TK_MAX_NODE_OUTPUTS] = {};
};

static int run_node(Node& n, hipStream_t s) {
  const tk_node& d = n.desc;
  const tk_tensor* i0 = &n.in[0].t;
  const tk_tensor* i1 = &n.in[1].t;
  const tk_tensor* i2 = &n.in[2].t;
  tk_tensor* o = &n.out[0].t;
  switch (d.kind) {
    case TK_NODE_CONV_BLOCK: {
      tk_block_attrs at = d.attrs.block;
      if (at.has_add) at.residual = &n.in[3].t;  // the module's own copy of the descriptor
      return conv2d_block_impl(i0, d.ext[0], i1, d.ext[1], (const int32_t*)d.ext[2], i2, n.outp, d.n_outputs, &at,
                               d.ext[3], d.ext[4], s);
    }
    case TK_NODE_DENSE_BLOCK:
      return dense_block_impl(i0, i1, i2, n.outp, d.n_outputs, &d.attrs.block, d.ext[0], s);
    case TK_NODE_CONV2D:
      return conv2d_prepared_impl(i0, d.ext[0], i1, d.ext[1], (const int32_t*)d.ext[2], o, &d.attrs.conv2d, d.ext[3], s);
    case TK_NODE_DENSE:
      return dense_impl(i0, i1, o, &d.attrs.dense, d.ext[0], s);
    case TK_NODE_REQUANTIZE:
      return requantize_impl(i0, o, &d.attrs.requantize, s);
    case TK_NODE_BIAS_ADD:
      return bias_add_impl(i0, i1, o, d.attrs.bias_add.axis, s);
    case TK_NODE_CLIP:
      return clip_impl(i0, o, d.attrs.clip.a_min, d.attrs.clip.a_max, s);
    case TK_NODE_CAST:
      return cast_impl(i0, o, s);
    case TK_NODE_QNN_ADD:
      return qnn_add_impl(i0, i1, o, &d.attrs.qnn_add, s);
    case TK_NODE_ADD_BLOCK:
      return add_block_impl(i0, i1, n.outp, d.n_outputs, &d.attrs.add_block, d.ext[4], s);
    case TK_NODE_MAX_POOL2D:
      if (d.ext[0]) return max_pool_shadow_impl(i0, d.ext[0], o, &d.attrs.pool2d, d.ext[4], s);
      if (d.ext[4]) {
        int rc = max_pool_impl(i0, o, &d.attrs.pool2d, s);
        return rc ? rc : make_shadow_impl(o, d.ext[4], s);
      }
      return max_pool_impl(i0, o, &d.attrs.pool2d, s);
    case TK_NODE_AVG_POOL2D:
      return avg_pool_impl(i0, o, &d.attrs.pool2d, s);
    case TK_NODE_GLOBAL_AVG_POOL2D:
      return global_avg_pool_impl(i0, o, s);
    case TK_NODE_COPY:
      return copy_impl(i0, o, s);
    case TK_NODE_SHADOW:
      return make_shadow_impl(i0, d.ext[0], s);
    case TK_NODE_POSTOPS:
      return postops_impl(i0, d.n_inputs > 1 ? i1 : nullptr, o, &d.attrs.postops, s);
    case TK_NODE_EWISE:
      return ewise_impl(i0, d.n_inputs > 1 ? i1 : nullptr, o, &d.attrs.ewise, s);
    case TK_NODE_CONV2D_F32:
      return conv2d_f32_impl(i0, i1, o, &d.attrs.conv2d, s);
    case TK_NODE_DENSE_F32:
      return dense_f32_impl(i0, i1, o, s);
    case TK_NODE_PAD:
      return pad_impl(i0, o, &d.attrs.pad, s);
    case TK_NODE_QUANTIZE:
      return qnn_quantize_impl(i0, o, &d.attrs.qparams, s);
    case TK_NODE_DEQUANTIZE:
      return qnn_dequantize_impl(i0, o, &d.attrs.qparams, s);
    case TK_NODE_QNN_BINARY:
      return qnn_binary_impl(i0, i1, o, &d.attrs.qnn_binary, s);
    case TK_NODE_CONCAT: {
      const tk_tensor* xs[TK_MAX_NODE_INPUTS];
      for (int k = 0; k < d.n_inputs; ++k) xs[k] = &n.in[k].t;
      return qnn_concatenate_impl(xs, d.n_inputs, o, &d.attrs.concat, s);
    }
    case TK_NODE_TRANSPOSE:
      return transpose_impl(i0, o, &d.attrs.transpose, s);
    case TK_NODE_LEAKY_RELU:
      return qnn_leaky_relu_impl(i0, o, &d.attrs.leaky_relu, s);
    case TK_NODE_LOOKUP:
      return qnn_lookup_impl(i0, o, d.ext[0], s);
    case TK_NODE_BATCH_MATMUL:
      return batch_matmul_impl(i0, i1, o, &d.attrs.dense, d.ext[0], s);
    case TK_NODE_CONV2D_TRANSPOSE:
      return qnn_conv2d_transpose_impl(i0, i1, o, &d.attrs.conv2d_transpose, s);
    case TK_NODE_SIM_QUANTIZE:
    case TK_NODE_SIM_DEQUANTIZE:
      return qnn_simulated_impl(d.kind == TK_NODE_SIM_QUANTIZE, i0, o, &d.attrs.simq, s);
    case TK_NODE_REQUANTIZE_FP:
      return requantize_fp_impl(i0, o, &d.attrs.requantize_fp, s);
    case TK_NODE_QNN_BINARY_FP:
      return qnn_binary_fp_impl(i0, i1, o, &d.attrs.qnn_binary_fp, s);
  }
  set_error("tk_module: unknown node kind " + std::to_string(d.kind));
  return TK_ERR_INVALID_ARG;
}

}  // namespace tk

// Packed trace capture for tk_module_run_graph (the default graph copy mode): the node outputs that
// have host destinations are gathered, chunk by chunk, into a device mirror of the host image range
// they span (header bytes included, loaded once from the host image), and each chunk is copied to
// host memory by ONE host-issued hipMemcpyAsync gated on an event recorded after the graph that
// ends with the chunk's pack kernel (one graph per chunk).  Two mirrors alternate between runs, so a run's kernels overlap the previous
// run's copies (only the pack into a mirror waits for that mirror's last copies).
struct PackRecHost {
  const void* src;
  int64_t dst, bytes, first_blk;
};
struct PackPlan {
  std::vector<void*> dst;         // host_dst this plan was built for (the cache key)
  char* host_lo = nullptr;        // mirrored host range [host_lo, host_lo + span)
  int64_t span = 0;
  void* mirror[2] = {nullptr, nullptr};
  struct Chunk {
    int after_node;               // pack + event after this node
    int64_t off, len;             // mirror range copied to host_lo + off
    int64_t table_off;            // first entry in `table`
    int n_rec;
    int64_t blocks;
  };
  std::vector<Chunk> chunks;
  void* table = nullptr;          // device PackRec entries of every chunk
  std::vector<hipEvent_t> ev[2];  // per chunk, recorded after its graph
  hipEvent_t mirror_done[2] = {nullptr, nullptr};
  bool mirror_used[2] = {false, false};
  std::vector<hipGraph_t> g[2];   // per mirror: one graph per chunk (+ a tail graph)
  std::vector<hipGraphExec_t> ge[2];
  int next = 0;
  // Trace wire (tk_module_set_trace_wire): the int32 records of a chunk, and its 1-byte records that
  // are clips of the record before them, are not packed; an encode kernel writes them into a pinned
  // slot and a host function widens the slot into the image.
  bool wire = false;
  struct Range {
    int64_t off, len;
  };
  struct WireCall {  // what one decode host function works on
    tk::WireJob job;
    std::atomic<int>* failed = nullptr;
  };
  struct WireChunk {
    std::vector<Range> raw;  // mirror ranges of the records that are not coded (runs of adjacent ones)
    int64_t seg_off = 0;     // first entry in `wire_segs`
    int64_t coded_bytes = 0, bound = 0;
    std::vector<tk::WireSegHost> segs;
    std::vector<tk::WireUnit> units;
    std::unique_ptr<WireCall[]> calls;  // one per slot
    hipEvent_t landed = nullptr;        // the chunk's wire work is done
    int last_slot = -1;
  };
  std::vector<WireChunk> wchunks;
  void* wire_segs = nullptr;   // device WireSegDev entries of every chunk
  // Bias coding: the bias vectors of the records coded with an addend, copied once when the plan
  // is built.  The encoder subtracts the device copy and the decoder adds the host copy, which is
  // a copy of that device copy; neither reads a node's live bias, so new parameters can make the
  // prediction worse but never the two sides disagree.
  int32_t* addend_dev = nullptr;
  std::vector<int32_t> addend_host;
  std::vector<void*> slots;    // pinned ring of worst-case-sized chunk slots
  uint32_t* cursors = nullptr; // device, one per slot
  std::vector<hipEvent_t> slot_done;  // decode of the slot's last use (decode stream)
  std::vector<char> slot_used;
  int slot_next = 0;
  ~PackPlan() {
    for (auto& w : wchunks)
      if (w.landed) (void)hipEventDestroy(w.landed);
    for (auto e : slot_done) (void)hipEventDestroy(e);
    for (void* p : slots) (void)hipHostFree(p);
    if (wire_segs) (void)hipFree(wire_segs);
    if (addend_dev) (void)hipFree(addend_dev);
    if (cursors) (void)hipFree(cursors);
    for (int m = 0; m < 2; ++m) {
      for (auto x : ge[m]) (void)hipGraphExecDestroy(x);
      for (auto x : g[m]) (void)hipGraphDestroy(x);
      for (auto e : ev[m]) (void)hipEventDestroy(e);
      if (mirror_done[m]) (void)hipEventDestroy(mirror_done[m]);
      if (mirror[m]) (void)hipFree(mirror[m]);
    }
    if (table) (void)hipFree(table);
  }
};

struct tk_module {
  std::vector<tk::Node> nodes;
  std::vector<hipEvent_t> done;  // one per node, recorded after it on the compute stream
  std::vector<hipEvent_t> prof;  // n+1 timing events for run_profiled / profiling mode
  // Recorded on the capture stream after the last D2H copy of a traced run.  Every later
  // run (and, through tk_module_wait_capture, every input write) first makes its stream wait
  // on it: the copies read the module's buffers, so overwriting them before the copies land
  // would mix two runs in one trace image (write-after-read across streams).
  hipEvent_t capture_done = nullptr;
  bool capture_recorded = false;
  bool capture_plain = false;  // the last capture copied from the record buffers themselves
  bool profiling = false;
  bool have_times = false;
  // tk_module_run_graph: the whole run (every node, and the copies when capturing) as one HIP
  // graph per (stream, capture stream, host destinations), instantiated once and replayed; a few
  // are kept (a file sink alternates two trace images)
  struct Graph {
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    hipStream_t s = nullptr, cs = nullptr;
    std::vector<void*> dst;
  };
  std::vector<Graph> graphs;
  hipEvent_t graph_join = nullptr, graph_pre = nullptr;
  // the graphs are captured on two streams of the module's own (the caller's may be the legacy
  // default stream, which cannot capture) and launched on the caller's
  hipStream_t cap_s = nullptr, cap_cs = nullptr, cap_cx[3] = {nullptr, nullptr, nullptr};
  // graph copies as copy kernels instead of memcpy nodes: measured slower (41.7 vs 52.7 GB/s per
  // traced ResNet-50 step, profiles/r03n_run_modes.txt), so off by default
  bool graph_copy_kernels = false;
  // memcpy nodes in this many parallel chains (1..4): 4 measured 53.4 GB/s per traced ResNet-50
  // step against 52.7 for one chain (profiles/r03s_graph_copy_chains.txt)
  int graph_copy_chains = 4;
  // packed capture (default): records gathered into device mirrors, copied in this many chunks
  bool graph_packed = true;
  int pack_chunks = 8;
  std::vector<std::unique_ptr<PackPlan>> packs;
  // copy trace of packed runs (tk_module_set_copy_trace): a timing event on the compute stream
  // before the run's first launch, and two per chunk on the capture stream around its copy
  bool copy_trace = false;
  hipEvent_t ct_t0 = nullptr;
  std::vector<hipEvent_t> ct_ev;
  std::vector<int64_t> ct_bytes;
  // trace wire of the packed capture: on unless TK_TRACE_WIRE=0 was set when the module was
  // created; wire traffic and decodes run on two streams of the module's own
  // TK_WIRE_CLAMP=0 at creation keeps the clip records raw (the same library's comparison run)
  // TK_WIRE_BIAS=0 at creation keeps the bias_add records plain differences (likewise)
  bool trace_wire = true, wire_forced_off = false, wire_clamp = true, wire_bias = true;
  hipStream_t wire_s = nullptr, dec_s = nullptr;
  hipEvent_t wire_tail = nullptr, decode_tail = nullptr;  // last wire work / decode of the last wire run
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
    void* dev = nullptr;  // ChainDev[n_chains] | tk_wire_mismatch[ops.size()]
    tk_wire_mismatch* report = nullptr;
  } chains;
  void drop_graph() {
    last_wire_plan = nullptr;
    for (Graph& x : graphs) {
      if (x.ge) (void)hipGraphExecDestroy(x.ge);
      if (x.g) (void)hipGraphDestroy(x.g);
    }
    graphs.clear();
    if (!packs.empty()) (void)hipDeviceSynchronize();  // their mirrors may still be copied from
    packs.clear();
  }
  ~tk_module() {
    drop_graph();
    if (chains.dev) (void)hipFree(chains.dev);
    for (auto e : done) (void)hipEventDestroy(e);
    for (auto e : prof) (void)hipEventDestroy(e);
    if (capture_done) (void)hipEventDestroy(capture_done);
    if (graph_join) (void)hipEventDestroy(graph_join);
    if (graph_pre) (void)hipEventDestroy(graph_pre);
    if (ct_t0) (void)hipEventDestroy(ct_t0);
    for (auto e : ct_ev) (void)hipEventDestroy(e);
    if (wire_tail) (void)hipEventDestroy(wire_tail);
    if (decode_tail) (void)hipEventDestroy(decode_tail);
    if (wire_s) (void)hipStreamDestroy(wire_s);
    if (dec_s) (void)hipStreamDestroy(dec_s);
    if (cap_s) (void)hipStreamDestroy(cap_s);
    if (cap_cs) (void)hipStreamDestroy(cap_cs);
    for (hipStream_t x : cap_cx)
      if (x) (void)hipStreamDestroy(x);
  }
};

// The stream about to write the module's buffers waits for the last traced run's copies.
static int wait_capture(tk_module* mod, hipStream_t s) {
  if (mod->capture_recorded) TK_HIP(hipStreamWaitEvent(s, mod->capture_done, 0));
  return TK_OK;
}

extern "C" {

// ---------------------------------------------------------------- per-op API
int64_t tk_conv2d_packed_weight_bytes(const tk_tensor* weight, int groups) {
  return tk::conv_packed_weight_bytes(weight, groups);
}
int tk_conv2d_pack_weight(const tk_tensor* weight, int groups, void* packed, int32_t* weight_sums, void* stream) {
  return tk::conv_pack_weight(weight, groups, packed, weight_sums, tk::as_stream(stream));
}
int64_t tk_conv2d_shadow_bytes(const tk_tensor* data) { return tk::conv_shadow_bytes(data); }
int64_t tk_conv2d_scratch_bytes(const tk_tensor* data, const tk_tensor* weight, const tk_conv2d_attrs* attrs,
                                int block) {
  return tk::conv_scratch_bytes(data, weight, attrs, block);
}
int tk_conv2d_make_shadow(const tk_tensor* data, void* shadow, void* stream) {
  return tk::make_shadow_impl(data, shadow, tk::as_stream(stream));
}
int tk_qnn_conv2d_prepared(const tk_tensor* data, const void* shadow, const tk_tensor* weight, const void* packed,
                           const int32_t* weight_sums, tk_tensor* out, const tk_conv2d_attrs* attrs, void* scratch,
                           void* stream) {
  return tk::conv2d_prepared_impl(data, shadow, weight, packed, weight_sums, out, attrs, scratch,
                                  tk::as_stream(stream));
}
int64_t tk_qnn_conv2d_workspace_bytes(const tk_tensor* data, const tk_tensor* weight, const tk_conv2d_attrs* attrs) {
  return tk::conv2d_workspace_bytes(data, weight, attrs);
}
int tk_qnn_conv2d(const tk_tensor* data, const tk_tensor* weight, tk_tensor* out, const tk_conv2d_attrs* attrs,
                  void* workspace, void* stream) {
  return tk::conv2d_impl(data, weight, out, attrs, workspace, tk::as_stream(stream));
}
int64_t tk_qnn_dense_workspace_bytes(const tk_tensor* data, const tk_tensor* weight) {
  return tk::dense_workspace_bytes(data, weight);
}
int tk_qnn_dense(const tk_tensor* data, const tk_tensor* weight, tk_tensor* out, const tk_dense_attrs* attrs,
                 void* workspace, void* stream) {
  return tk::dense_impl(data, weight, out, attrs, workspace, tk::as_stream(stream));
}
int tk_qnn_conv2d_block(const tk_tensor* data, const void* shadow, const tk_tensor* weight, const void* packed,
                        const int32_t* weight_sums, const tk_tensor* bias, tk_tensor* const* outs, int n_outs,
                        const tk_block_attrs* attrs, void* scratch, void* shadow_out, void* stream) {
  return tk::conv2d_block_impl(data, shadow, weight, packed, weight_sums, bias, outs, n_outs, attrs, scratch,
                               shadow_out, tk::as_stream(stream));
}
int tk_conv2d_block_algos(const tk_tensor* data, const tk_tensor* weight, const tk_block_attrs* attrs,
                          int32_t* algos, int max_algos) {
  return tk::conv2d_block_algos_impl(data, weight, attrs, algos, max_algos);
}
int tk_conv2d_block_algo_info(const tk_tensor* data, const tk_tensor* weight, const tk_block_attrs* attrs, int algo,
                              char* buf, int len) {
  return tk::conv2d_block_algo_info_impl(data, weight, attrs, algo, buf, len);
}
int tk_qnn_dense_block(const tk_tensor* data, const tk_tensor* weight, const tk_tensor* bias, tk_tensor* const* outs,
                       int n_outs, const tk_block_attrs* attrs, void* workspace, void* stream) {
  return tk::dense_block_impl(data, weight, bias, outs, n_outs, attrs, workspace, tk::as_stream(stream));
}
int tk_requantize(const tk_tensor* data, tk_tensor* out, const tk_requantize_attrs* attrs, void* stream) {
  return tk::requantize_impl(data, out, attrs, tk::as_stream(stream));
}
int tk_qnn_add_block(const tk_tensor* lhs, const tk_tensor* rhs, tk_tensor* const* outs, int n_outs,
                     const tk_add_block_attrs* attrs, void* shadow_out, void* stream) {
  return tk::add_block_impl(lhs, rhs, outs, n_outs, attrs, shadow_out, tk::as_stream(stream));
}
int tk_qnn_add(const tk_tensor* lhs, const tk_tensor* rhs, tk_tensor* out, const tk_qnn_add_attrs* attrs,
               void* stream) {
  return tk::qnn_add_impl(lhs, rhs, out, attrs, tk::as_stream(stream));
}
int tk_bias_add(const tk_tensor* data, const tk_tensor* bias, tk_tensor* out, int axis, void* stream) {
  return tk::bias_add_impl(data, bias, out, axis, tk::as_stream(stream));
}
int tk_clip(const tk_tensor* data, tk_tensor* out, int64_t a_min, int64_t a_max, void* stream) {
  return tk::clip_impl(data, out, a_min, a_max, tk::as_stream(stream));
}
int tk_cast(const tk_tensor* data, tk_tensor* out, void* stream) {
  return tk::cast_impl(data, out, tk::as_stream(stream));
}
int tk_max_pool2d(const tk_tensor* data, tk_tensor* out, const tk_pool2d_attrs* attrs, void* stream) {
  return tk::max_pool_impl(data, out, attrs, tk::as_stream(stream));
}
int tk_max_pool2d_shadow(const tk_tensor* data, const void* data_shadow, tk_tensor* out,
                         const tk_pool2d_attrs* attrs, void* out_shadow, void* stream) {
  return tk::max_pool_shadow_impl(data, data_shadow, out, attrs, out_shadow, tk::as_stream(stream));
}
int tk_avg_pool2d(const tk_tensor* data, tk_tensor* out, const tk_pool2d_attrs* attrs, void* stream) {
  return tk::avg_pool_impl(data, out, attrs, tk::as_stream(stream));
}
int tk_global_avg_pool2d(const tk_tensor* data, tk_tensor* out, void* stream) {
  return tk::global_avg_pool_impl(data, out, tk::as_stream(stream));
}
int tk_copy(const tk_tensor* data, tk_tensor* out, void* stream) {
  return tk::copy_impl(data, out, tk::as_stream(stream));
}
int tk_pad(const tk_tensor* data, tk_tensor* out, const tk_pad_attrs* attrs, void* stream) {
  return tk::pad_impl(data, out, attrs, tk::as_stream(stream));
}
int tk_tachikoma_postops(const tk_tensor* acc, const tk_tensor* sum_src, tk_tensor* out,
                         const tk_postops_attrs* attrs, void* stream) {
  return tk::postops_impl(acc, sum_src, out, attrs, tk::as_stream(stream));
}
int tk_ewise(const tk_tensor* x, const tk_tensor* rhs, tk_tensor* out, const tk_ewise_attrs* attrs, void* stream) {
  return tk::ewise_impl(x, rhs, out, attrs, tk::as_stream(stream));
}
int tk_conv2d_f32(const tk_tensor* data, const tk_tensor* weight, tk_tensor* out, const tk_conv2d_attrs* attrs,
                  void* stream) {
  return tk::conv2d_f32_impl(data, weight, out, attrs, tk::as_stream(stream));
}
int tk_dense_f32(const tk_tensor* data, const tk_tensor* weight, tk_tensor* out, void* stream) {
  return tk::dense_f32_impl(data, weight, out, tk::as_stream(stream));
}
int64_t tk_qnn_batch_matmul_workspace_bytes(const tk_tensor* x, const tk_tensor* y) {
  return tk::batch_matmul_workspace_bytes(x, y);
}
int tk_qnn_batch_matmul(const tk_tensor* x, const tk_tensor* y, tk_tensor* out, const tk_dense_attrs* attrs,
                        void* workspace, void* stream) {
  return tk::batch_matmul_impl(x, y, out, attrs, workspace, tk::as_stream(stream));
}

// ---------------------------------------------------------------- executor
int tk_module_create(const tk_node* nodes, int n_nodes, tk_module** out) {
  if (!out || n_nodes < 0 || (n_nodes > 0 && !nodes)) {
    tk::set_error("tk_module_create: invalid argument");
    return TK_ERR_INVALID_ARG;
  }
  auto mod = std::make_unique<tk_module>();
  if (const char* e = std::getenv("TK_TRACE_WIRE")) mod->wire_forced_off = e[0] == '0' && e[1] == 0;
  if (const char* e = std::getenv("TK_WIRE_CLAMP")) mod->wire_clamp = !(e[0] == '0' && e[1] == 0);
  if (const char* e = std::getenv("TK_WIRE_BIAS")) mod->wire_bias = !(e[0] == '0' && e[1] == 0);
  mod->nodes.resize(n_nodes);
  for (int i = 0; i < n_nodes; ++i) {
    const tk_node& src = nodes[i];
    tk::Node& dst = mod->nodes[i];
    dst.desc = src;
    if (src.n_inputs < 0 || src.n_inputs > TK_MAX_NODE_INPUTS) {
      tk::set_error("tk_module_create: node " + std::to_string(i) + " has a bad input count");
      return TK_ERR_INVALID_ARG;
    }
    if (src.kind == TK_NODE_CONV_BLOCK && src.attrs.block.has_add && src.n_inputs != 4) {
      tk::set_error("tk_module_create: node " + std::to_string(i) + ": a residual block takes the residual as input 3");
      return TK_ERR_INVALID_ARG;
    }
    for (int k = 0; k < src.n_inputs; ++k) {
      if (!src.inputs[k]) {
        tk::set_error("tk_module_create: node " + std::to_string(i) + " has a null input");
        return TK_ERR_INVALID_ARG;
      }
      dst.in[k].assign(src.inputs[k]);
    }
    if (src.n_outputs < 0 || src.n_outputs > TK_MAX_NODE_OUTPUTS || (src.kind != TK_NODE_SHADOW && src.n_outputs < 1)) {
      tk::set_error("tk_module_create: node " + std::to_string(i) + " has a bad output count");
      return TK_ERR_INVALID_ARG;
    }
    for (int k = 0; k < src.n_outputs; ++k) {
      if (!src.outputs[k]) {
        tk::set_error("tk_module_create: node " + std::to_string(i) + " has a null output");
        return TK_ERR_INVALID_ARG;
      }
      dst.out[k].assign(src.outputs[k]);
    }
    for (int k = 0; k < TK_MAX_NODE_INPUTS; ++k) dst.desc.inputs[k] = nullptr;  // resolved through dst.in / dst.out
    for (int k = 0; k < TK_MAX_NODE_OUTPUTS; ++k) dst.desc.outputs[k] = nullptr;
  }
  for (auto& n : mod->nodes)
    for (int k = 0; k < TK_MAX_NODE_OUTPUTS; ++k) n.outp[k] = &n.out[k].t;
  mod->done.resize(n_nodes);
  for (int i = 0; i < n_nodes; ++i) {
    hipError_t e = hipEventCreateWithFlags(&mod->done[i], hipEventDisableTiming);
    if (e != hipSuccess) {
      mod->done.resize(i);
      tk::set_error(std::string("tk_module_create: hipEventCreate failed: ") + hipGetErrorString(e));
      return TK_ERR_HIP;
    }
  }
  {
    hipError_t e = hipEventCreateWithFlags(&mod->capture_done, hipEventDisableTiming);
    if (e != hipSuccess) {
      mod->capture_done = nullptr;
      tk::set_error(std::string("tk_module_create: hipEventCreate failed: ") + hipGetErrorString(e));
      return TK_ERR_HIP;
    }
  }
  *out = mod.release();
  return TK_OK;
}

int tk_module_destroy(tk_module* mod) {
  delete mod;
  return TK_OK;
}

int tk_module_num_nodes(const tk_module* mod) { return mod ? (int)mod->nodes.size() : 0; }

static int ensure_prof_events(tk_module* mod) {
  while (mod->prof.size() < mod->nodes.size() + 1) {
    hipEvent_t e;
    TK_HIP(hipEventCreate(&e));
    mod->prof.push_back(e);
  }
  return TK_OK;
}

int tk_module_set_profiling(tk_module* mod, int enable) {
  if (!mod) {
    tk::set_error("tk_module_set_profiling: null module");
    return TK_ERR_INVALID_ARG;
  }
  mod->profiling = enable != 0;
  mod->have_times = false;
  return mod->profiling ? ensure_prof_events(mod) : TK_OK;
}

int tk_module_node_times(tk_module* mod, float* node_ms) {
  if (!mod || !node_ms || !mod->have_times) {
    tk::set_error("tk_module_node_times: no profiled run recorded");
    return TK_ERR_INVALID_ARG;
  }
  size_t n = mod->nodes.size();
  TK_HIP(hipEventSynchronize(mod->prof[n]));
  for (size_t i = 0; i < n; ++i) TK_HIP(hipEventElapsedTime(&node_ms[i], mod->prof[i], mod->prof[i + 1]));
  return TK_OK;
}

// Enqueues every node on s and, when capturing, node i's output copies on cs gated by an event
// recorded after node i (shared by tk_module_run and the graph capture of tk_module_run_graph).
static int enqueue_nodes(tk_module* mod, hipStream_t s, hipStream_t cs, void* const* host_dst, bool capture,
                         bool profiling, bool copy_kernels = false, hipStream_t const* chains = nullptr,
                         int n_chains = 1, int* n_copied = nullptr) {
  if (profiling) TK_HIP(hipEventRecord(mod->prof[0], s));
  int copied = 0;  // captured nodes so far: node copies rotate over the chains
  if (n_copied) *n_copied = 0;
  for (size_t i = 0; i < mod->nodes.size(); ++i) {
    tk::Node& n = mod->nodes[i];
    int rc = tk::run_node(n, s);
    if (rc) {
      tk::set_error("node " + std::to_string(i) + ": " + tk_last_error());
      return rc;
    }
    if (profiling) TK_HIP(hipEventRecord(mod->prof[i + 1], s));
    if (capture && n.desc.n_outputs > 0) {
      void* const* dst = host_dst + i * TK_MAX_NODE_OUTPUTS;
      bool any = false;
      for (int k = 0; k < n.desc.n_outputs; ++k) any |= dst[k] != nullptr;
      if (any) {
        if (chains) cs = chains[copied % n_chains];
        ++copied;
        if (n_copied) *n_copied = copied;
        TK_HIP(hipEventRecord(mod->done[i], s));
        TK_HIP(hipStreamWaitEvent(cs, mod->done[i], 0));
        if (copy_kernels) {
          // one copy kernel for the node's records (graph runs: a kernel node, no host call)
          const void* src[TK_MAX_NODE_OUTPUTS];
          int64_t nb[TK_MAX_NODE_OUTPUTS];
          for (int k = 0; k < n.desc.n_outputs; ++k) src[k] = tk::ptr(&n.out[k].t), nb[k] = tk::nbytes(&n.out[k].t);
          int rc = tk::host_copy_impl(src, dst, nb, n.desc.n_outputs, cs);
          if (rc) return rc;
        } else {
          for (int k = 0; k < n.desc.n_outputs; ++k)
            if (dst[k])
              TK_HIP(hipMemcpyAsync(dst[k], tk::ptr(&n.out[k].t), tk::nbytes(&n.out[k].t), hipMemcpyDeviceToHost, cs));
        }
      }
    }
  }
  return TK_OK;
}

int tk_module_run(tk_module* mod, void* stream, void* capture_stream, void* const* host_dst) {
  if (!mod) {
    tk::set_error("tk_module_run: null module");
    return TK_ERR_INVALID_ARG;
  }
  hipStream_t s = tk::as_stream(stream);
  hipStream_t cs = tk::as_stream(capture_stream);
  bool capture = capture_stream && host_dst;
  int rc0 = wait_capture(mod, s);
  if (rc0) return rc0;
  rc0 = enqueue_nodes(mod, s, cs, host_dst, capture, mod->profiling);
  if (rc0) return rc0;
  if (capture) {
    // the next run / input write waits for these copies (wait_capture)
    TK_HIP(hipEventRecord(mod->capture_done, cs));
    mod->capture_recorded = true;
    mod->capture_plain = true;
  }
  mod->have_times = mod->profiling;
  return TK_OK;
}

int tk_module_set_graph_copies(tk_module* mod, int copy_kernels) {
  if (!mod || copy_kernels < 0 || copy_kernels > 5) {
    tk::set_error("tk_module_set_graph_copies: invalid argument");
    return TK_ERR_INVALID_ARG;
  }
  const bool packed = copy_kernels == 0;
  const bool kern = copy_kernels == 1;
  const int chains = copy_kernels == 5 ? 1 : copy_kernels >= 2 ? std::min(copy_kernels, 4) : 1;
  if (mod->graph_packed != packed || mod->graph_copy_kernels != kern || mod->graph_copy_chains != chains)
    mod->drop_graph();
  mod->graph_packed = packed;
  mod->graph_copy_kernels = kern;
  mod->graph_copy_chains = chains;
  return TK_OK;
}

int tk_module_set_trace_chunks(tk_module* mod, int chunks) {
  if (!mod || chunks < 1 || chunks > 256) {
    tk::set_error("tk_module_set_trace_chunks: chunks must be 1..256");
    return TK_ERR_INVALID_ARG;
  }
  if (mod->pack_chunks != chunks) mod->drop_graph();
  mod->pack_chunks = chunks;
  return TK_OK;
}

// The steps of build_pack_plan.  A record of the plan: a node output that has a host destination.
struct PackRecord {
  char* host;
  const void* src;
  int64_t bytes;
  int node, out;
  const tk_tensor* t;
  bool wire, diff;  // coded on the wire; as the difference from the record before it
  bool clamp;       // coded on the wire as a clamp of the record before it (1-byte)
  // a differenced record that is the bias_add of the record before it: the bias vector, the
  // geometry of its axis and where its snapshot lies in the plan's addend buffers (int32 elements)
  const tk_tensor* bias = nullptr;
  int32_t plane = 0, channels = 0;
  int64_t addend_at = 0;
};

// the records in host order; overlapping destinations are refused
static int collect_records(const tk_module* mod, const std::vector<void*>& dst, std::vector<PackRecord>* recs) {
  for (size_t i = 0; i < mod->nodes.size(); ++i) {
    const tk::Node& n = mod->nodes[i];
    for (int k = 0; k < n.desc.n_outputs; ++k) {
      char* h = (char*)dst[i * TK_MAX_NODE_OUTPUTS + k];
      const int64_t nb = tk::nbytes(&n.out[k].t);
      if (h && nb > 0) recs->push_back({h, tk::ptr(&n.out[k].t), nb, (int)i, k, &n.out[k].t, false, false, false});
    }
  }
  std::sort(recs->begin(), recs->end(), [](const PackRecord& a, const PackRecord& b) { return a.host < b.host; });
  for (size_t r = 0; r + 1 < recs->size(); ++r)
    if ((*recs)[r].host + (*recs)[r].bytes > (*recs)[r + 1].host) {
      tk::set_error("tk_module_run_graph: overlapping record destinations");
      return TK_ERR_INVALID_ARG;
    }
  return TK_OK;
}

// the tensor that output k of node n clips, where the node declares that output as a clip
static const void* clip_input(const tk::Node& n, int k) {
  const tk_node& d = n.desc;
  const bool block = d.kind == TK_NODE_CONV_BLOCK || d.kind == TK_NODE_DENSE_BLOCK;
  if ((block && d.attrs.block.has_clip) || (d.kind == TK_NODE_ADD_BLOCK && d.attrs.add_block.has_clip))
    return k >= 1 && k == d.n_outputs - 1 ? tk::ptr(&n.out[k - 1].t) : nullptr;
  return d.kind == TK_NODE_CLIP && k == 0 ? tk::ptr(&n.in[0].t) : nullptr;
}

// The bias that output k of node n adds to the tensor at `from`, where the node declares that
// output as the bias_add of that tensor: output 1 of a conv or dense block over its output 0, or a
// TK_NODE_BIAS_ADD over its input.  *axis: the record's axis the bias runs along.
static const tk_tensor* bias_input(const tk::Node& n, int k, const void* from, int* axis) {
  const tk_node& d = n.desc;
  if ((d.kind == TK_NODE_CONV_BLOCK || d.kind == TK_NODE_DENSE_BLOCK) && k == 1 && d.n_inputs >= 3 &&
      tk::ptr(&n.out[0].t) == from) {
    *axis = d.kind == TK_NODE_CONV_BLOCK ? 1 : n.out[1].t.ndim - 1;
    return &n.in[2].t;
  }
  if (d.kind == TK_NODE_BIAS_ADD && k == 0 && d.n_inputs >= 2 && tk::ptr(&n.in[0].t) == from) {
    *axis = d.attrs.bias_add.axis < 0 ? d.attrs.bias_add.axis + n.out[0].t.ndim : d.attrs.bias_add.axis;
    return &n.in[1].t;
  }
  return nullptr;
}

// int32 records are coded; one that follows (in the image) a coded record of its own shape is
// coded as the difference from it (every bias_add after its convolution), and where its node
// declares it as the bias_add of that record, with a compact int32 bias of the axis' length and
// fewer than 2^31 elements, as the difference less the bias (tk_wire.h: bias coding; the values are
// a snapshot the plan takes, never the live tensor; TK_WIRE_BIAS=0 keeps plain differences).  A compact 1-byte
// record that its node declares as the clip of the record before it in the image (same dtype
// and shape) is coded as a clamp of that record; every other 1-byte record stays raw.  Returns
// whether any record is coded.
static bool decide_coding(const tk_module* mod, std::vector<PackRecord>& recs) {
  bool any = false;
  for (size_t r = 0; r < recs.size(); ++r) {
    PackRecord& c = recs[r];
    const tk_tensor* a = c.t;
    const tk_tensor* b = r ? recs[r - 1].t : nullptr;
    const bool same_shape = b && a->ndim == b->ndim && std::equal(a->shape, a->shape + a->ndim, b->shape);
    if (mod->wire_clamp && tk::is_int8ish(a) && tk::compact(a) && same_shape && tk::compact(b) &&
        a->dtype.code == b->dtype.code && b->dtype.bits == 8 && b->dtype.lanes == 1 && c.src != recs[r - 1].src &&
        clip_input(mod->nodes[c.node], c.out) == recs[r - 1].src) {
      c.wire = c.clamp = any = true;
      continue;
    }
    c.wire = tk::is_int(c.t, 32) && tk::compact(c.t) && ((uintptr_t)c.src & 3) == 0;
    any |= c.wire;
    if (!c.wire || r == 0 || !recs[r - 1].wire) continue;
    c.diff = same_shape && tk::is_int(b, 32) && c.src != recs[r - 1].src;
    int axis = 0;
    const tk_tensor* bias = c.diff && mod->wire_bias ? bias_input(mod->nodes[c.node], c.out, recs[r - 1].src, &axis) : nullptr;
    if (!bias || !bias->data || axis < 0 || axis >= a->ndim || !tk::is_int(bias, 32) || !tk::compact(bias) ||
        tk::numel(bias) != a->shape[axis] || a->shape[axis] < 1 || a->shape[axis] >= ((int64_t)1 << 31) ||
        tk::numel(a) >= ((int64_t)1 << 31))
      continue;
    int64_t plane = 1;
    for (int d = axis + 1; d < a->ndim; ++d) plane *= a->shape[d];
    c.bias = bias, c.plane = (int32_t)plane, c.channels = (int32_t)a->shape[axis];
  }
  return any;
}

// A chunk's wire tables, planned by tk::wire_plan from its coded records (`coded`: their indices in
// `recs`): the encoder's segments (record buffers on the device), the host decoder's (image bytes),
// the decode units and the size of a slot with every block raw.
static int chunk_wire_tables(const std::vector<PackRecord>& recs, const std::vector<size_t>& coded, const PackPlan* plan,
                             PackPlan::WireChunk* wc, std::vector<tk::WireSegDev>& wire_segs) {
  std::vector<tk_wire_record> wrecs;  // offsets are not used here
  for (size_t q = 0; q < coded.size(); ++q) {
    const PackRecord& r = recs[coded[q]];
    // a record follows its predecessor in the decode order only where that one is coded in this
    // chunk too (a difference, or a clamp of a clamp); an earlier chunk's record, or a raw
    // predecessor, has landed by then
    const bool chained = (r.diff || r.clamp) && q > 0 && coded[q - 1] == coded[q] - 1;
    const int esize = tk::elem_bytes(r.t);
    wrecs.push_back({0, r.bytes / esize, chained, esize == 4 ? tk::kWireI32 : tk::is_int(r.t, 8) ? tk::kWireI8 : tk::kWireU8});
  }
  tk::WirePlan wp;
  if (const int rc = tk::wire_plan(wrecs.data(), (int)wrecs.size(), -1, "tk_module_run_graph", &wp)) return rc;
  wc->units = std::move(wp.units);
  wc->seg_off = (int64_t)wire_segs.size();
  wc->bound = wp.bound;
  for (const tk::WireSegRef& sr : wp.segs) {
    const PackRecord& r = recs[coded[sr.rec]];
    // a differenced record's predecessor is the record before it in the image (this chunk's
    // or, for the chunk's first record, an earlier chunk's: decoded before this one)
    const PackRecord* pv = r.diff || r.clamp ? &recs[coded[sr.rec] - 1] : nullptr;
    const int kind = wrecs[sr.rec].kind;
    const tk::WireSegAddr dev = tk::wire_seg_addr(sr, kind, r.src, pv ? pv->src : nullptr);
    const tk::WireSegAddr img = tk::wire_seg_addr(sr, kind, r.host, pv ? pv->host : nullptr);
    wire_segs.push_back({dev.at, dev.prev, sr.n, kind});
    wc->segs.push_back({img.at, img.prev, sr.n, kind});
    if (r.bias) {  // each side is handed its own copy of the plan's snapshot
      tk::wire_seg_bias(&wire_segs.back(), plan->addend_dev + r.addend_at, r.plane, r.channels, sr.e0);
      tk::wire_seg_bias(&wc->segs.back(), plan->addend_host.data() + r.addend_at, r.plane, r.channels, sr.e0);
    }
  }
  for (size_t q : coded) wc->coded_bytes += recs[q].bytes;
  return TK_OK;
}

// The plan's snapshot of the bias vectors its records are coded with (PackPlan::addend_dev /
// addend_host): each vector copied device to device into one buffer, and that buffer to the host.
static int snapshot_addends(PackPlan* plan, std::vector<PackRecord>& recs) {
  int64_t total = 0;
  for (PackRecord& r : recs)
    if (r.bias) r.addend_at = total, total += r.channels;
  if (!total) return TK_OK;
  TK_HIP(hipMalloc((void**)&plan->addend_dev, (size_t)total * sizeof(int32_t)));
  for (const PackRecord& r : recs)
    if (r.bias)
      TK_HIP(hipMemcpy(plan->addend_dev + r.addend_at, tk::ptr(r.bias), (size_t)r.channels * sizeof(int32_t),
                       hipMemcpyDeviceToDevice));
  plan->addend_host.resize((size_t)total);
  TK_HIP(hipMemcpy(plan->addend_host.data(), plan->addend_dev, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost));
  return TK_OK;
}

// The chunks, cut at node boundaries where every record below the cut is written, with the pack
// table and, on the wire, each chunk's raw ranges and wire tables.
static int cut_chunks(const tk_module* mod, const std::vector<PackRecord>& recs, PackPlan* plan,
                      std::vector<PackRecHost>& table, std::vector<tk::WireSegDev>& wire_segs) {
  // after node i, every record below complete_upto[i] (host order) is written
  const int nn = (int)mod->nodes.size();
  std::vector<int64_t> complete_upto(nn);
  std::vector<int> prefix_max(recs.size());  // max producer node among records [0, q]
  for (size_t q = 0; q < recs.size(); ++q) prefix_max[q] = std::max(q ? prefix_max[q - 1] : -1, recs[q].node);
  for (int i = 0, r = 0; i < nn; ++i) {
    while (r < (int)recs.size() && prefix_max[r] <= i) ++r;
    complete_upto[i] = r == (int)recs.size() ? plan->span : recs[r].host - plan->host_lo;
  }
  const int64_t target = std::max<int64_t>(1, (plan->span + mod->pack_chunks - 1) / mod->pack_chunks);
  int64_t cut = 0;
  size_t next_rec = 0;
  for (int i = 0; i < nn; ++i) {
    const int64_t upto = complete_upto[i];
    if (upto <= cut) continue;
    if (upto - cut < target && upto < plan->span) continue;
    PackPlan::Chunk c{i, cut, upto - cut, (int64_t)table.size(), 0, 0};
    int64_t blocks = 0;
    PackPlan::WireChunk wc;
    std::vector<size_t> w_rec;  // the chunk's coded records
    bool in_run = false;  // the previous record of this chunk was not coded
    while (next_rec < recs.size() && recs[next_rec].host - plan->host_lo < upto) {
      const PackRecord& rc = recs[next_rec++];
      const int64_t off = rc.host - plan->host_lo;
      if (rc.wire) {
        w_rec.push_back(next_rec - 1);
        in_run = false;
        continue;
      }
      if (plan->wire) {
        if (in_run) wc.raw.back().len = off + rc.bytes - wc.raw.back().off;
        else wc.raw.push_back({off, rc.bytes});
        in_run = true;
      }
      const int64_t a0 = off & ~(int64_t)15;
      const int64_t nblk = (off + rc.bytes - a0 + 256 * 16 - 1) / (256 * 16);
      table.push_back({rc.src, off, rc.bytes, blocks});
      blocks += nblk;
      ++c.n_rec;
    }
    c.blocks = blocks;
    plan->chunks.push_back(c);
    cut = upto;
    if (!plan->wire) continue;
    if (!w_rec.empty())
      if (const int rc = chunk_wire_tables(recs, w_rec, plan, &wc, wire_segs)) return rc;
    plan->wchunks.push_back(std::move(wc));
  }
  if (cut != plan->span || next_rec != recs.size()) {
    tk::set_error("tk_module_run_graph: pack plan does not cover every record");
    return TK_ERR_INVALID_ARG;
  }
  return TK_OK;
}

// The device pack table, two mirrors and their events; on the wire also the device segment table,
// a ring of pinned slots each large enough for any chunk with every block raw, a cursor per slot,
// the decode calls of every (chunk, slot) pair and the module's streams.
static int alloc_pack_resources(tk_module* mod, PackPlan* plan, const std::vector<PackRecHost>& table,
                                const std::vector<tk::WireSegDev>& wire_segs) {
  if (!table.empty()) {
    TK_HIP(hipMalloc(&plan->table, table.size() * sizeof(PackRecHost)));
    TK_HIP(hipMemcpy(plan->table, table.data(), table.size() * sizeof(PackRecHost), hipMemcpyHostToDevice));
  }
  if (plan->wire) {
    TK_HIP(hipMalloc(&plan->wire_segs, wire_segs.size() * sizeof(tk::WireSegDev)));
    TK_HIP(hipMemcpy(plan->wire_segs, wire_segs.data(), wire_segs.size() * sizeof(tk::WireSegDev), hipMemcpyHostToDevice));
    int64_t slot_bytes = 0;
    int coded_chunks = 0;
    for (const auto& w : plan->wchunks) slot_bytes = std::max(slot_bytes, w.bound), coded_chunks += !w.segs.empty();
    const int n_slots = std::min(3, coded_chunks);
    for (int k = 0; k < n_slots; ++k) {
      void* p = nullptr;
      TK_HIP(hipHostMalloc(&p, (size_t)slot_bytes, hipHostMallocDefault));
      plan->slots.push_back(p);
      hipEvent_t e;
      TK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      plan->slot_done.push_back(e);
    }
    plan->slot_used.assign(n_slots, 0);
    TK_HIP(hipMalloc((void**)&plan->cursors, n_slots * sizeof(uint32_t)));
    for (auto& w : plan->wchunks) {
      if (w.segs.empty()) continue;
      TK_HIP(hipEventCreateWithFlags(&w.landed, hipEventDisableTiming));
      w.calls.reset(new PackPlan::WireCall[n_slots]);
      for (int k = 0; k < n_slots; ++k) {
        tk::WireJob& j = w.calls[k].job;
        j.wire = (const char*)plan->slots[k];
        j.wire_bytes = w.bound;
        j.segs = w.segs.data(), j.n_seg = (int64_t)w.segs.size();
        j.units = w.units.data(), j.n_units = (int64_t)w.units.size();
        w.calls[k].failed = &mod->wire_failed;
      }
    }
    if (!mod->wire_s) TK_HIP(hipStreamCreateWithFlags(&mod->wire_s, hipStreamNonBlocking));
    if (!mod->dec_s) TK_HIP(hipStreamCreateWithFlags(&mod->dec_s, hipStreamNonBlocking));
    if (!mod->wire_tail) TK_HIP(hipEventCreateWithFlags(&mod->wire_tail, hipEventDisableTiming));
    if (!mod->decode_tail) TK_HIP(hipEventCreateWithFlags(&mod->decode_tail, hipEventDisableTiming));
  }
  for (int m = 0; m < 2; ++m) {
    // the mirror holds the image's bytes between records (headers) from the start
    TK_HIP(hipMalloc(&plan->mirror[m], (size_t)plan->span + 16));
    TK_HIP(hipMemcpy(plan->mirror[m], plan->host_lo, (size_t)plan->span, hipMemcpyHostToDevice));
    TK_HIP(hipEventCreateWithFlags(&plan->mirror_done[m], hipEventDisableTiming));
    plan->ev[m].resize(plan->chunks.size(), nullptr);
    for (auto& e : plan->ev[m]) TK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  if (!mod->cap_s) TK_HIP(hipStreamCreateWithFlags(&mod->cap_s, hipStreamNonBlocking));
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
        rc = tk::run_node(mod->nodes[i], qs);
        if (rc) tk::set_error("node " + std::to_string(i) + ": " + tk_last_error());
      }
      if (rc == TK_OK && has_chunk && plan->chunks[seg].n_rec > 0) {
        const PackPlan::Chunk& ch = plan->chunks[seg];
        rc = tk::pack_records_impl((const char*)plan->table + ch.table_off * sizeof(PackRecHost), ch.n_rec, ch.blocks,
                                   plan->mirror[m], qs);
      }
      hipGraph_t g = nullptr;
      hipError_t e = hipStreamEndCapture(qs, &g);
      if (rc) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
      }
      if (e != hipSuccess || !g) {
        (void)hipGetLastError();
        tk::set_error(std::string("tk_module_run_graph: stream capture failed: ") + hipGetErrorString(e));
        return TK_ERR_HIP;
      }
      plan->g[m].push_back(g);
      hipGraphExec_t ge = nullptr;
      e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
      if (e != hipSuccess) {
        tk::set_error(std::string("tk_module_run_graph: instantiate failed: ") + hipGetErrorString(e));
        return TK_ERR_HIP;
      }
      plan->ge[m].push_back(ge);
    }
  }
  return TK_OK;
}

// Builds the packed-capture plan for host destinations `dst`: the mirrored range, the chunks (cut
// at node boundaries where every record below the cut is written), the device pack tables, two
// mirrors loaded with the host image's bytes, and one graph per chunk and mirror.
static int build_pack_plan(tk_module* mod, const std::vector<void*>& dst, PackPlan** out) {
  auto plan = std::make_unique<PackPlan>();
  plan->dst = dst;
  std::vector<PackRecord> recs;
  if (const int rc = collect_records(mod, dst, &recs)) return rc;
  if (recs.empty()) {
    *out = nullptr;
    return TK_OK;
  }
  plan->wire = mod->trace_wire && !mod->wire_forced_off && decide_coding(mod, recs);
  plan->host_lo = recs.front().host;
  plan->span = recs.back().host + recs.back().bytes - plan->host_lo;
  std::vector<PackRecHost> table;
  std::vector<tk::WireSegDev> wire_segs;
  if (plan->wire)
    if (const int rc = snapshot_addends(plan.get(), recs)) return rc;
  if (const int rc = cut_chunks(mod, recs, plan.get(), table, wire_segs)) return rc;
  if (const int rc = alloc_pack_resources(mod, plan.get(), table, wire_segs)) return rc;
  if (const int rc = capture_chunk_graphs(mod, plan.get())) return rc;
  *out = plan.release();
  return TK_OK;
}

// The decode host function of one chunk (decode stream): widens the chunk's slot into the image
// on the decoder's pool and waits for it; no HIP call.
static void wire_decode_call(void* p) {
  auto* call = static_cast<PackPlan::WireCall*>(p);
  if (tk::wire_decode(&call->job, 0)) call->failed->store(1);
}

// The wire side of one chunk of a packed run, after the chunk's graph and its event on s:
//   s       graph c | ev ................ graph c+1 | ev ...
//   wire_s  wait ev, wait slot_done[k] | cursor = 0 | encode -> slot k | raw copies | landed[c]
//   dec_s   wait landed[c] | host function: decode slot k -> image | slot_done[k]
static int enqueue_wire_chunk(tk_module* mod, PackPlan* plan, int m, size_t c, bool trace) {
  const PackPlan::Chunk& ch = plan->chunks[c];
  PackPlan::WireChunk& w = plan->wchunks[c];
  hipStream_t ws = mod->wire_s, ds = mod->dec_s;
  TK_HIP(hipStreamWaitEvent(ws, plan->ev[m][c], 0));
  if (trace) TK_HIP(hipEventRecord(mod->ct_ev[2 * c], ws));
  int k = -1;
  if (!w.segs.empty()) {
    k = plan->slot_next;
    plan->slot_next = (k + 1) % (int)plan->slots.size();
    if (plan->slot_used[k]) TK_HIP(hipStreamWaitEvent(ws, plan->slot_done[k], 0));
    TK_HIP(hipMemsetAsync(plan->cursors + k, 0, sizeof(uint32_t), ws));
    const int rc = tk::wire_encode_impl((const tk::WireSegDev*)plan->wire_segs + w.seg_off, (int64_t)w.segs.size(),
                                        plan->cursors + k, plan->slots[k], w.bound, ws);
    if (rc) return rc;
  }
  for (const PackPlan::Range& r : w.raw)
    TK_HIP(hipMemcpyAsync(plan->host_lo + r.off, (char*)plan->mirror[m] + r.off, (size_t)r.len, hipMemcpyDeviceToHost, ws));
  if (trace) {
    TK_HIP(hipEventRecord(mod->ct_ev[2 * c + 1], ws));
    mod->ct_bytes[c] = ch.len;
  }
  if (k >= 0) {
    TK_HIP(hipEventRecord(w.landed, ws));
    TK_HIP(hipStreamWaitEvent(ds, w.landed, 0));
    TK_HIP(hipLaunchHostFunc(ds, wire_decode_call, &w.calls[k]));
    TK_HIP(hipEventRecord(plan->slot_done[k], ds));
    plan->slot_used[k] = 1;
    w.last_slot = k;
  }
  return TK_OK;
}

// One packed traced run: the chunk graphs of mirror m (kernels, pack kernel) on s, each followed by
// an event, and the chunk copies on cs, each after its event (wire runs: enqueue_wire_chunk).
static int run_packed(tk_module* mod, hipStream_t s, hipStream_t cs, void* const* host_dst) {
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
    if (!built) return tk::TK_OK_RUN;  // nothing to capture
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
    tk::set_error("tk_module_run_graph: a wire buffer of an earlier run did not decode");
    return TK_ERR_INVALID_ARG;
  }
  // the encode kernels of the last wire run read the record buffers this run overwrites
  if (mod->wire_tail_used) TK_HIP(hipStreamWaitEvent(s, mod->wire_tail, 0));
  const bool trace = mod->copy_trace;
  if (trace) {
    if (!mod->ct_t0) TK_HIP(hipEventCreate(&mod->ct_t0));
    while (mod->ct_ev.size() < 2 * plan->chunks.size()) {
      hipEvent_t e;
      TK_HIP(hipEventCreate(&e));
      mod->ct_ev.push_back(e);
    }
    mod->ct_bytes.assign(plan->chunks.size(), 0);
    TK_HIP(hipEventRecord(mod->ct_t0, s));
  }
  for (size_t c = 0; c < plan->ge[m].size(); ++c) {
    TK_HIP(hipGraphLaunch(plan->ge[m][c], s));
    if (c >= plan->chunks.size()) break;  // the tail graph
    const PackPlan::Chunk& ch = plan->chunks[c];
    TK_HIP(hipEventRecord(plan->ev[m][c], s));
    if (plan->wire) {
      const int rc = enqueue_wire_chunk(mod, plan, m, c, trace);
      if (rc) return rc;
      continue;
    }
    TK_HIP(hipStreamWaitEvent(cs, plan->ev[m][c], 0));
    if (trace) TK_HIP(hipEventRecord(mod->ct_ev[2 * c], cs));
    TK_HIP(hipMemcpyAsync(plan->host_lo + ch.off, (char*)plan->mirror[m] + ch.off, (size_t)ch.len,
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
    const PackPlan::WireChunk& w = plan->wchunks[c];
    const tk::WireJob* j = w.last_slot >= 0 ? &w.calls[w.last_slot].job : nullptr;
    int64_t raw = 0;
    for (const PackPlan::Range& r : w.raw) raw += r.len;
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

int tk_module_run_graph(tk_module* mod, void* stream, void* capture_stream, void* const* host_dst) {
  if (!mod) {
    tk::set_error("tk_module_run_graph: null module");
    return TK_ERR_INVALID_ARG;
  }
  if (mod->profiling) return tk_module_run(mod, stream, capture_stream, host_dst);  // per-node events
  hipStream_t s = tk::as_stream(stream);
  hipStream_t cs = tk::as_stream(capture_stream);
  const bool capture = capture_stream && host_dst;
  if (capture && mod->graph_packed) {
    const int rc = run_packed(mod, s, cs, host_dst);
    if (rc != tk::TK_OK_RUN) {
      mod->have_times = false;
      return rc;
    }
    // no record has a host destination: an ordinary graph run below
  }
  const size_t nd = capture ? mod->nodes.size() * TK_MAX_NODE_OUTPUTS : 0;
  std::vector<void*> dst(nd);
  for (size_t i = 0; i < nd; ++i) dst[i] = host_dst[i];
  int gi = -1;
  for (size_t i = 0; i < mod->graphs.size(); ++i)
    if (mod->graphs[i].dst == dst && (mod->graphs[i].cs != nullptr) == capture) gi = (int)i;
  int rc0 = wait_capture(mod, s);
  if (rc0) return rc0;
  if (gi < 0) {
    if (mod->graphs.size() >= 4) {  // keep the newest few
      tk_module::Graph& old = mod->graphs.front();
      if (old.ge) (void)hipGraphExecDestroy(old.ge);
      if (old.g) (void)hipGraphDestroy(old.g);
      mod->graphs.erase(mod->graphs.begin());
    }
    if (!mod->graph_join) TK_HIP(hipEventCreateWithFlags(&mod->graph_join, hipEventDisableTiming));
    if (!mod->cap_s) TK_HIP(hipStreamCreateWithFlags(&mod->cap_s, hipStreamNonBlocking));
    if (!mod->cap_cs) TK_HIP(hipStreamCreateWithFlags(&mod->cap_cs, hipStreamNonBlocking));
    hipStream_t qs = mod->cap_s, qcs = mod->cap_cs;
    hipStream_t chains[4] = {qcs, nullptr, nullptr, nullptr};
    const int nch = capture ? mod->graph_copy_chains : 1;
    for (int c = 1; c < nch; ++c) {
      if (!mod->cap_cx[c - 1]) TK_HIP(hipStreamCreateWithFlags(&mod->cap_cx[c - 1], hipStreamNonBlocking));
      chains[c] = mod->cap_cx[c - 1];
    }
    // capture: the node loop on qs, the copies forked onto qcs through the per-node events and
    // joined back into qs at the end, so that one launch covers the run and its copies
    TK_HIP(hipStreamBeginCapture(qs, hipStreamCaptureModeThreadLocal));
    int copied = 0;
    int rc = enqueue_nodes(mod, qs, qcs, host_dst, capture, false, mod->graph_copy_kernels, chains, nch, &copied);
    // a chain enters the capture only once a node's copy was routed to it: join only those
    // (joining an idle chain would record on a stream that is not capturing)
    const int joined = std::min(copied, nch);
    for (int c = 0; c < joined && rc == TK_OK && capture; ++c) {
      // every copy chain joins back into qs (one event per join: record, then wait, in order)
      if (hipEventRecord(mod->graph_join, chains[c]) != hipSuccess || hipStreamWaitEvent(qs, mod->graph_join, 0) != hipSuccess) {
        tk::set_error("tk_module_run_graph: joining the capture streams failed");
        rc = TK_ERR_HIP;
      }
    }
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(qs, &g);
    if (rc) {
      if (g) (void)hipGraphDestroy(g);
      return rc;
    }
    if (e != hipSuccess || !g) {
      (void)hipGetLastError();
      tk::set_error(std::string("tk_module_run_graph: stream capture failed: ") + hipGetErrorString(e));
      return TK_ERR_HIP;
    }
    hipGraphExec_t ge = nullptr;
    e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
      (void)hipGraphDestroy(g);
      tk::set_error(std::string("tk_module_run_graph: instantiate failed: ") + hipGetErrorString(e));
      return TK_ERR_HIP;
    }
    tk_module::Graph x;
    x.g = g;
    x.ge = ge;
    x.s = qs;
    x.cs = capture ? qcs : nullptr;
    x.dst = std::move(dst);
    mod->graphs.push_back(std::move(x));
    gi = (int)mod->graphs.size() - 1;
  }
  if (capture) {
    // whatever the caller queued on the capture stream before this run (the graph-input copies)
    // completes before the launch, so that capture_done covers it as in tk_module_run
    if (!mod->graph_pre) TK_HIP(hipEventCreateWithFlags(&mod->graph_pre, hipEventDisableTiming));
    TK_HIP(hipEventRecord(mod->graph_pre, cs));
    TK_HIP(hipStreamWaitEvent(s, mod->graph_pre, 0));
  }
  TK_HIP(hipGraphLaunch(mod->graphs[gi].ge, s));
  if (capture) {
    // the next run / input write waits for this run's copies (they are part of the launch on s),
    // and so does the capture stream: as after tk_module_run, work queued on it later (or its
    // synchronisation) sees the copies complete
    TK_HIP(hipEventRecord(mod->capture_done, s));
    mod->capture_recorded = true;
    mod->capture_plain = true;
    TK_HIP(hipStreamWaitEvent(cs, mod->capture_done, 0));
  }
  mod->have_times = false;
  return TK_OK;
}

int tk_module_wait_capture(tk_module* mod, void* stream) {
  if (!mod) {
    tk::set_error("tk_module_wait_capture: null module");
    return TK_ERR_INVALID_ARG;
  }
  return wait_capture(mod, tk::as_stream(stream));
}

int tk_module_run_range(tk_module* mod, int begin, int end, void* stream) {
  if (!mod || begin < 0 || end > (int)mod->nodes.size() || begin > end) {
    tk::set_error("tk_module_run_range: bad range");
    return TK_ERR_INVALID_ARG;
  }
  hipStream_t s = tk::as_stream(stream);
  int rc0 = wait_capture(mod, s);
  if (rc0) return rc0;
  for (int i = begin; i < end; ++i) {
    int rc = tk::run_node(mod->nodes[i], s);
    if (rc) return rc;
  }
  return TK_OK;
}

int tk_module_run_order(tk_module* mod, const int32_t* order, int n, void* stream) {
  if (!mod || n < 0 || (n > 0 && !order)) {
    tk::set_error("tk_module_run_order: null module, negative count or null order");
    return TK_ERR_INVALID_ARG;
  }
  for (int k = 0; k < n; ++k)
    if (order[k] < 0 || order[k] >= (int)mod->nodes.size()) {
      tk::set_error("tk_module_run_order: node index " + std::to_string(order[k]) + " out of range");
      return TK_ERR_INVALID_ARG;
    }
  hipStream_t s = tk::as_stream(stream);
  int rc0 = wait_capture(mod, s);
  if (rc0) return rc0;
  for (int k = 0; k < n; ++k) {
    int rc = tk::run_node(mod->nodes[order[k]], s);
    if (rc) return rc;
  }
  return TK_OK;
}

// Lays out the chain table of the module's conv, dense and add blocks and puts it on the device.
static int build_chains(tk_module* mod, hipStream_t s) {
  tk_module::Chains& c = mod->chains;
  std::vector<tk::ChainDev> table;
  std::vector<tk_chain_op> ops;
  int n_report = 0;
  int64_t blocks = 0;
  for (size_t i = 0; i < mod->nodes.size(); ++i) {
    tk::Node& n = mod->nodes[i];
    const tk_node& d = n.desc;
    if (d.kind != TK_NODE_CONV_BLOCK && d.kind != TK_NODE_DENSE_BLOCK && d.kind != TK_NODE_ADD_BLOCK) continue;
    tk::ChainSpec sp{};
    sp.kind = d.kind;
    sp.outs = n.outp;
    sp.n_outs = d.n_outputs;
    if (d.kind == TK_NODE_ADD_BLOCK) {
      sp.add_block = &d.attrs.add_block;
    } else {
      sp.bias = &n.in[2].t;
      sp.block = &d.attrs.block;
      if (d.attrs.block.has_add) sp.residual = &n.in[3].t;
    }
    const int before = n_report;
    if (const int rc = tk::chain_append(sp, "tk_module_check_chains", &table, &n_report, &blocks)) return rc;
    // the tail ops write outputs 1 .. n_outputs - 1 of the node, in chain order
    for (int k = 0; k < n_report - before; ++k) ops.push_back({(int32_t)i, d.n_outputs - (n_report - before) + k});
  }
  if (blocks >= ((int64_t)1 << 31)) {
    tk::set_error("tk_module_check_chains: too much to check in one launch");
    return TK_ERR_UNSUPPORTED;
  }
  if (!table.empty()) {
    const int64_t table_bytes = tk::wire_align((int64_t)(table.size() * sizeof(tk::ChainDev)), 64);
    TK_HIP(hipMalloc(&c.dev, (size_t)(table_bytes + n_report * (int64_t)sizeof(tk_wire_mismatch))));
    c.report = (tk_wire_mismatch*)((char*)c.dev + table_bytes);
    // once per module: wait, so that the table is there whichever stream a later call uses
    TK_HIP(hipMemcpyAsync(c.dev, table.data(), table.size() * sizeof(tk::ChainDev), hipMemcpyHostToDevice, s));
    TK_HIP(hipStreamSynchronize(s));
  }
  c.n_chains = (int)table.size();
  c.blocks = blocks;
  c.ops = std::move(ops);
  c.built = true;
  return TK_OK;
}

int tk_module_chain_ops(tk_module* mod, tk_chain_op* ops, int capacity) {
  if (!mod || capacity < 0 || (capacity > 0 && !ops)) {
    tk::set_error("tk_module_chain_ops: null module or null array");
    return TK_ERR_INVALID_ARG;
  }
  if (!mod->chains.built)
    if (const int rc = build_chains(mod, nullptr)) return rc;
  const int n = (int)mod->chains.ops.size();
  for (int k = 0; k < std::min(n, capacity); ++k) ops[k] = mod->chains.ops[k];
  return n;
}

int tk_module_check_chains(tk_module* mod, tk_wire_mismatch* report, int capacity, void* stream) {
  if (!mod || !report || capacity < 0) {
    tk::set_error("tk_module_check_chains: null module or null report");
    return TK_ERR_INVALID_ARG;
  }
  hipStream_t s = tk::as_stream(stream);
  tk_module::Chains& c = mod->chains;
  if (!c.built)
    if (const int rc = build_chains(mod, s)) return rc;
  const int n = (int)c.ops.size();
  if (n > capacity) {
    tk::set_error("tk_module_check_chains: the report holds " + std::to_string(capacity) + " entries, the module has " +
                  std::to_string(n) + " tail ops (tk_module_chain_ops)");
    return TK_ERR_INVALID_ARG;
  }
  for (int k = 0; k < n; ++k) report[k].mismatches = 0, report[k].first = ~(uint64_t)0;
  if (c.n_chains == 0) return n;
  if (const int rc = tk::chain_check_impl((const tk::ChainDev*)c.dev, c.n_chains, c.blocks, c.report, n, s)) return rc;
  TK_HIP(hipMemcpyAsync(report, c.report, (size_t)n * sizeof(tk_wire_mismatch), hipMemcpyDeviceToHost, s));
  // the report is filled once the call's own work on `stream` is complete, as tk_compare_device_batch's
  if (hipStreamSynchronize(s) != hipSuccess) {
    tk::set_error("tk_module_check_chains: the chain-check kernel failed");
    return TK_ERR_HIP;
  }
  return n;
}

int tk_module_run_profiled(tk_module* mod, void* stream, float* node_ms) {
  if (!mod || !node_ms) {
    tk::set_error("tk_module_run_profiled: invalid argument");
    return TK_ERR_INVALID_ARG;
  }
  size_t n = mod->nodes.size();
  int rc0 = ensure_prof_events(mod);
  if (rc0) return rc0;
  hipStream_t s = tk::as_stream(stream);
  rc0 = wait_capture(mod, s);
  if (rc0) return rc0;
  TK_HIP(hipEventRecord(mod->prof[0], s));
  for (size_t i = 0; i < n; ++i) {
    int rc = tk::run_node(mod->nodes[i], s);
    if (rc) return rc;
    TK_HIP(hipEventRecord(mod->prof[i + 1], s));
  }
  TK_HIP(hipEventSynchronize(mod->prof[n]));
  for (size_t i = 0; i < n; ++i) TK_HIP(hipEventElapsedTime(&node_ms[i], mod->prof[i], mod->prof[i + 1]));
  return TK_OK;
}

// Shape + attribute key of a conv-block node: nodes with equal keys run the same kernels on the
// same amount of work, so one measurement serves all of them.
static std::string tune_key(const tk::Node& n) {
  const tk_node& d = n.desc;
  const tk_block_attrs& b = d.attrs.block;
  std::string k;
  auto add = [&](int64_t v) { k += std::to_string(v) + ","; };
  for (int i = 0; i < 2; ++i) {
    const tk_tensor& t = n.in[i].t;
    add(t.dtype.code), add(t.dtype.bits);
    for (int j = 0; j < t.ndim; ++j) add(t.shape[j]);
    k += "|";
  }
  for (int v : b.conv.strides) add(v);
  for (int v : b.conv.padding) add(v);
  for (int v : b.conv.dilation) add(v);
  add(b.conv.groups), add(b.conv.input_zero_point), add(b.conv.kernel_zero_point), add(b.conv.kernel_zero_points != nullptr);
  add(b.requantize.mode), add(b.has_clip), add(b.has_add), add(d.n_outputs), add(d.ext[4] != nullptr);
  return k;
}

int tk_module_set_node_algo(tk_module* mod, int node, int algo) {
  if (!mod || node < 0 || node >= (int)mod->nodes.size()) {
    tk::set_error("tk_module_set_node_algo: bad node");
    return TK_ERR_INVALID_ARG;
  }
  tk::Node& n = mod->nodes[node];
  if (n.desc.kind != TK_NODE_CONV_BLOCK) {
    tk::set_error("tk_module_set_node_algo: node " + std::to_string(node) + " is not a conv block");
    return TK_ERR_INVALID_ARG;
  }
  if (algo != 0) {
    std::vector<int32_t> algos(256, -1);
    const int total = tk_conv2d_block_algos(&n.in[0].t, &n.in[1].t, &n.desc.attrs.block, algos.data(), 256);
    if (total < 0) return total;
    if (std::find(algos.begin(), algos.begin() + std::min(total, 256), algo) == algos.begin() + std::min(total, 256)) {
      tk::set_error("tk_module_set_node_algo: algo " + std::to_string(algo) + " is not a candidate of node " +
                    std::to_string(node) + " (tk_conv2d_block_algos)");
      return TK_ERR_INVALID_ARG;
    }
  }
  if (n.desc.attrs.block.algo != algo) mod->drop_graph();  // captured graphs hold the old kernel
  n.desc.attrs.block.algo = algo;
  return TK_OK;
}

int tk_module_tune(tk_module* mod, void* stream, int max_candidates, int reps, int32_t* algo_out, float* us_out) {
  if (!mod || max_candidates < 1 || reps < 1) {
    tk::set_error("tk_module_tune: invalid argument");
    return TK_ERR_INVALID_ARG;
  }
  hipStream_t s = tk::as_stream(stream);
  mod->drop_graph();  // the kernels it captured may change
  const int W = max_candidates + 1;
  const size_t n = mod->nodes.size();
  if (algo_out)
    for (size_t i = 0; i < n * W; ++i) algo_out[i] = -1;
  if (us_out)
    for (size_t i = 0; i < n * W; ++i) us_out[i] = -1.0f;
  int rc0 = wait_capture(mod, s);
  if (rc0) return rc0;
  hipEvent_t e0, e1;
  TK_HIP(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    tk::set_error("tk_module_tune: hipEventCreate failed");
    return TK_ERR_HIP;
  }
  struct Result {
    int best;
    std::vector<int32_t> algos;
    std::vector<float> us;
  };
  std::map<std::string, Result> seen;
  int rc = TK_OK;
  // A residual-join node reads the qnn.add operand, which in the network is a record written
  // several kernels earlier and comes from HBM; timed back to back it stays in the MALL and the
  // kernels that expose its load latency look faster than they run (the 56x56 expand: 115 us
  // cached, 136-153 cold, profiles/r05x_residual_cold_vs_cached.txt).  So each of its timed
  // launches follows a 512 MiB fill of a scratch buffer that evicts the caches, and is timed alone.
  // If the device cannot spare the flush buffer (a module near the memory limit: packed mirrors
  // are up to 4 x 7.45 GB at batch 64), the buffer shrinks to a quarter of the free memory, and
  // below 64 MiB the node is timed warm, back to back like the others, instead of failing the tune.
  void* flush = nullptr;
  size_t flush_bytes = (size_t)512 << 20;
  bool flush_unavailable = false;
  auto timed_warm = [&](tk::Node& node, float* us) -> int {
    if (hipEventRecord(e0, s) != hipSuccess) return TK_ERR_HIP;
    for (int k = 0; k < reps; ++k) {
      const int r = tk::run_node(node, s);
      if (r) return r;
    }
    float ms = 0.0f;
    if (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
        hipEventElapsedTime(&ms, e0, e1) != hipSuccess)
      return TK_ERR_HIP;
    *us = ms * 1e3f / (float)reps;
    return TK_OK;
  };
  auto timed_cold = [&](tk::Node& node, float* us) -> int {
    if (!flush && !flush_unavailable && hipMalloc(&flush, flush_bytes) != hipSuccess) {
      flush = nullptr;
      (void)hipGetLastError();
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b / 4 >= ((size_t)64 << 20)) {
        flush_bytes = (free_b / 4) & ~(((size_t)1 << 20) - 1);
        if (hipMalloc(&flush, flush_bytes) != hipSuccess) {
          flush = nullptr;
          (void)hipGetLastError();
        }
      } else {
        (void)hipGetLastError();
      }
      flush_unavailable = flush == nullptr;
    }
    if (flush_unavailable) return timed_warm(node, us);
    float total = 0.0f;
    for (int k = 0; k < reps; ++k) {
      if (hipMemsetAsync(flush, k & 0xFF, flush_bytes, s) != hipSuccess || hipEventRecord(e0, s) != hipSuccess)
        return TK_ERR_HIP;
      const int r = tk::run_node(node, s);
      if (r) return r;
      float ms = 0.0f;
      if (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
          hipEventElapsedTime(&ms, e0, e1) != hipSuccess)
        return TK_ERR_HIP;
      total += ms;
    }
    *us = total * 1e3f / (float)reps;
    return TK_OK;
  };
  for (size_t i = 0; i < n && rc == TK_OK; ++i) {
    tk::Node& node = mod->nodes[i];
    if (node.desc.kind != TK_NODE_CONV_BLOCK) continue;
    const std::string key = tune_key(node);
    auto it = seen.find(key);
    if (it == seen.end()) {
      Result r{0, std::vector<int32_t>(max_candidates, -1), std::vector<float>(max_candidates, -1.0f)};
      int total = tk_conv2d_block_algos(&node.in[0].t, &node.in[1].t, &node.desc.attrs.block, r.algos.data(),
                                        max_candidates);
      if (total < 0) {
        rc = total;
        break;
      }
      float best_us = 0.0f;
      for (int c = 0; c < std::min(total, max_candidates) && rc == TK_OK; ++c) {
        node.desc.attrs.block.algo = r.algos[c];
        rc = tk::run_node(node, s);  // warm-up (and the image-tile kernel's LDS attribute)
        if (rc == TK_ERR_INVALID_ARG) {
          // a candidate this node's arguments rule out (refused before any launch): skip it
          rc = TK_OK;
          continue;
        }
        if (rc) break;
        rc = node.desc.attrs.block.has_add ? timed_cold(node, &r.us[c]) : timed_warm(node, &r.us[c]);
        if (rc) break;
        if (best_us <= 0.0f || r.us[c] < best_us) best_us = r.us[c], r.best = r.algos[c];
      }
      if (rc) {
        node.desc.attrs.block.algo = 0;
        if (rc == TK_ERR_HIP) tk::set_error("tk_module_tune: node " + std::to_string(i) + ": HIP timing failed");
        else tk::set_error("tk_module_tune: node " + std::to_string(i) + ": " + tk_last_error());
        break;
      }
      it = seen.emplace(key, std::move(r)).first;
    }
    const Result& r = it->second;
    node.desc.attrs.block.algo = r.best;
    if (algo_out) {
      algo_out[i * W] = r.best;
      for (int c = 0; c < max_candidates; ++c) algo_out[i * W + 1 + c] = r.algos[c];
    }
    if (us_out) {
      float b = -1.0f;
      for (int c = 0; c < max_candidates; ++c)
        if (r.algos[c] == r.best) b = r.us[c];
      us_out[i * W] = b;
      for (int c = 0; c < max_candidates; ++c) us_out[i * W + 1 + c] = r.us[c];
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (flush) {
    (void)hipStreamSynchronize(s);
    (void)hipFree(flush);
  }
  return rc;
}

}  // extern "C"
