// The planner of the packed trace capture (tk_capture_plan.h).  Plain C++: no HIP call, no HIP
// include; what it plans is allocated, captured and run by tk_capture.cc.
#include "tk_capture_plan.h"

#include <algorithm>

namespace tk {
namespace {

// the records in host order; overlapping destinations are refused
int collect_records(const std::vector<Node>& nodes, void* const* dst, std::vector<CaptureRecord>* recs) {
  for (size_t i = 0; i < nodes.size(); ++i) {
    const Node& n = nodes[i];
    for (int k = 0; k < n.desc.n_outputs; ++k) {
      char* h = (char*)dst[i * TK_MAX_NODE_OUTPUTS + k];
      const int64_t nb = nbytes(&n.out[k].t);
      if (h && nb > 0) recs->push_back({h, ptr(&n.out[k].t), nb, (int)i, k, &n.out[k].t, false, false, false});
    }
  }
  std::sort(recs->begin(), recs->end(), [](const CaptureRecord& a, const CaptureRecord& b) { return a.host < b.host; });
  for (size_t r = 0; r + 1 < recs->size(); ++r)
    if ((*recs)[r].host + (*recs)[r].bytes > (*recs)[r + 1].host) {
      set_error("tk_module_run_graph: overlapping record destinations");
      return TK_ERR_INVALID_ARG;
    }
  return TK_OK;
}

// the tensor that output k of node n clips, where the node declares that output as a clip
const void* clip_input(const Node& n, int k) {
  const tk_node& d = n.desc;
  const bool block = d.kind == TK_NODE_CONV_BLOCK || d.kind == TK_NODE_DENSE_BLOCK;
  if ((block && d.attrs.block.has_clip) || (d.kind == TK_NODE_ADD_BLOCK && d.attrs.add_block.has_clip))
    return k >= 1 && k == d.n_outputs - 1 ? ptr(&n.out[k - 1].t) : nullptr;
  return d.kind == TK_NODE_CLIP && k == 0 ? ptr(&n.in[0].t) : nullptr;
}

// The bias that output k of node n adds to the tensor at `from`, where the node declares that
// output as the bias_add of that tensor: output 1 of a conv or dense block over its output 0, or a
// TK_NODE_BIAS_ADD over its input.  *axis: the record's axis the bias runs along.
const tk_tensor* bias_input(const Node& n, int k, const void* from, int* axis) {
  const tk_node& d = n.desc;
  if ((d.kind == TK_NODE_CONV_BLOCK || d.kind == TK_NODE_DENSE_BLOCK) && k == 1 && d.n_inputs >= 3 &&
      ptr(&n.out[0].t) == from) {
    *axis = d.kind == TK_NODE_CONV_BLOCK ? 1 : n.out[1].t.ndim - 1;
    return &n.in[2].t;
  }
  if (d.kind == TK_NODE_BIAS_ADD && k == 0 && d.n_inputs >= 2 && ptr(&n.in[0].t) == from) {
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
bool decide_coding(const std::vector<Node>& nodes, const CaptureOptions& opt, std::vector<CaptureRecord>& recs) {
  bool any = false;
  for (size_t r = 0; r < recs.size(); ++r) {
    CaptureRecord& c = recs[r];
    const tk_tensor* a = c.t;
    const tk_tensor* b = r ? recs[r - 1].t : nullptr;
    const bool same_shape = b && a->ndim == b->ndim && std::equal(a->shape, a->shape + a->ndim, b->shape);
    if (opt.clamp && is_int8ish(a) && compact(a) && same_shape && compact(b) &&
        a->dtype.code == b->dtype.code && b->dtype.bits == 8 && b->dtype.lanes == 1 && c.src != recs[r - 1].src &&
        clip_input(nodes[c.node], c.out) == recs[r - 1].src) {
      c.wire = c.clamp = any = true;
      continue;
    }
    c.wire = is_int(c.t, 32) && compact(c.t) && ((uintptr_t)c.src & 3) == 0;
    any |= c.wire;
    if (!c.wire || r == 0 || !recs[r - 1].wire) continue;
    c.diff = same_shape && is_int(b, 32) && c.src != recs[r - 1].src;
    int axis = 0;
    const tk_tensor* bias = c.diff && opt.bias ? bias_input(nodes[c.node], c.out, recs[r - 1].src, &axis) : nullptr;
    if (!bias || !bias->data || axis < 0 || axis >= a->ndim || !is_int(bias, 32) || !compact(bias) ||
        numel(bias) != a->shape[axis] || a->shape[axis] < 1 || a->shape[axis] >= ((int64_t)1 << 31) ||
        numel(a) >= ((int64_t)1 << 31))
      continue;
    int64_t plane = 1;
    for (int d = axis + 1; d < a->ndim; ++d) plane *= a->shape[d];
    c.bias = bias, c.plane = (int32_t)plane, c.channels = (int32_t)a->shape[axis];
  }
  return any;
}

// A chunk's wire tables, planned by wire_plan from its coded records (`coded`: their indices in
// plan->recs): the encoder's segments (record buffers on the device), the host decoder's (image
// bytes), the decode units and the size of a slot with every block raw.
int chunk_wire_tables(const std::vector<size_t>& coded, const int32_t* addend_dev, const int32_t* addend_host,
                      CapturePlan* plan, CapturePlan::WireChunk* wc) {
  const std::vector<CaptureRecord>& recs = plan->recs;
  std::vector<tk_wire_record> wrecs;  // offsets are not used here
  for (size_t q = 0; q < coded.size(); ++q) {
    const CaptureRecord& r = recs[coded[q]];
    // a record follows its predecessor in the decode order only where that one is coded in this
    // chunk too (a difference, or a clamp of a clamp); an earlier chunk's record, or a raw
    // predecessor, has landed by then
    const bool chained = (r.diff || r.clamp) && q > 0 && coded[q - 1] == coded[q] - 1;
    const int esize = elem_bytes(r.t);
    wrecs.push_back({0, r.bytes / esize, chained, esize == 4 ? kWireI32 : is_int(r.t, 8) ? kWireI8 : kWireU8});
  }
  WirePlan wp;
  if (const int rc = wire_plan(wrecs.data(), (int)wrecs.size(), -1, "tk_module_run_graph", &wp)) return rc;
  wc->units = std::move(wp.units);
  wc->seg_off = (int64_t)plan->wire_segs.size();
  wc->bound = wp.bound;
  for (const WireSegRef& sr : wp.segs) {
    const CaptureRecord& r = recs[coded[sr.rec]];
    // a differenced record's predecessor is the record before it in the image (this chunk's
    // or, for the chunk's first record, an earlier chunk's: decoded before this one)
    const CaptureRecord* pv = r.diff || r.clamp ? &recs[coded[sr.rec] - 1] : nullptr;
    const int kind = wrecs[sr.rec].kind;
    const WireSegAddr dev = wire_seg_addr(sr, kind, r.src, pv ? pv->src : nullptr);
    const WireSegAddr img = wire_seg_addr(sr, kind, r.host, pv ? pv->host : nullptr);
    auto bias = [&](const int32_t* snapshot) {  // each side is handed its own copy of the plan's snapshot
      return wire_seg_bias(r.bias ? snapshot + r.addend_at : nullptr, r.plane, r.channels, sr.e0);
    };
    plan->wire_segs.push_back({dev.at, dev.prev, sr.n, kind, bias(addend_dev)});
    wc->segs.push_back({img.at, img.prev, sr.n, kind, bias(addend_host)});
  }
  for (size_t q : coded) wc->coded_bytes += recs[q].bytes;
  return TK_OK;
}

}  // namespace

int capture_plan_records(const std::vector<Node>& nodes, void* const* host_dst, const CaptureOptions& opt,
                         CapturePlan* plan) {
  std::vector<CaptureRecord>& recs = plan->recs;
  if (const int rc = collect_records(nodes, host_dst, &recs)) return rc;
  if (recs.empty()) return TK_OK;
  plan->wire = opt.wire && decide_coding(nodes, opt, recs);
  plan->host_lo = recs.front().host;
  plan->span = recs.back().host + recs.back().bytes - plan->host_lo;
  if (plan->wire)
    for (CaptureRecord& r : recs)
      if (r.bias) r.addend_at = plan->addend_total, plan->addend_total += r.channels;
  return TK_OK;
}

int capture_plan_chunks(int n_nodes, int chunks, const int32_t* addend_dev, const int32_t* addend_host,
                        CapturePlan* plan) {
  const std::vector<CaptureRecord>& recs = plan->recs;
  // after node i, every record below complete_upto[i] (host order) is written
  const int nn = n_nodes;
  std::vector<int64_t> complete_upto(nn);
  std::vector<int> prefix_max(recs.size());  // max producer node among records [0, q]
  for (size_t q = 0; q < recs.size(); ++q) prefix_max[q] = std::max(q ? prefix_max[q - 1] : -1, recs[q].node);
  for (int i = 0, r = 0; i < nn; ++i) {
    while (r < (int)recs.size() && prefix_max[r] <= i) ++r;
    complete_upto[i] = r == (int)recs.size() ? plan->span : recs[r].host - plan->host_lo;
  }
  const int64_t target = std::max<int64_t>(1, (plan->span + chunks - 1) / chunks);
  int64_t cut = 0;
  size_t next_rec = 0;
  for (int i = 0; i < nn; ++i) {
    const int64_t upto = complete_upto[i];
    if (upto <= cut) continue;
    if (upto - cut < target && upto < plan->span) continue;
    CapturePlan::Chunk c{i, cut, upto - cut, (int64_t)plan->table.size(), 0, 0};
    int64_t blocks = 0;
    CapturePlan::WireChunk wc;
    std::vector<size_t> w_rec;  // the chunk's coded records
    bool in_run = false;  // the previous record of this chunk was not coded
    while (next_rec < recs.size() && recs[next_rec].host - plan->host_lo < upto) {
      const CaptureRecord& rc = recs[next_rec++];
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
      plan->table.push_back({(const uint8_t*)rc.src, off, rc.bytes, blocks});
      blocks += pack_rec_blocks(off, rc.bytes);
      ++c.n_rec;
    }
    c.blocks = blocks;
    plan->chunks.push_back(c);
    cut = upto;
    if (!plan->wire) continue;
    if (!w_rec.empty())
      if (const int rc = chunk_wire_tables(w_rec, addend_dev, addend_host, plan, &wc)) return rc;
    plan->wchunks.push_back(std::move(wc));
  }
  if (cut != plan->span || next_rec != recs.size()) {
    set_error("tk_module_run_graph: pack plan does not cover every record");
    return TK_ERR_INVALID_ARG;
  }
  return TK_OK;
}

}  // namespace tk
