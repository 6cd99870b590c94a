// Stand-alone check of the packed capture's planner (csrc/tk_capture_plan.cc) for sanitizer builds:
// the chunks, the pack table, the raw ranges, every clause of the coding decisions, the wire
// segments and units (also of a chain cut by a chunk boundary) and the refusal, on node lists built
// by hand whose data pointers and image addresses are never dereferenced.  CPU only; never needs a
// device.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -I include \
//       tools/capture_plan_check.cc tachikoma_amd/csrc/tk_capture_plan.cc tachikoma_amd/csrc/tk_wire.cc \
//       -o capture_plan_check && ./capture_plan_check
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../tachikoma_amd/csrc/tk_capture_plan.h"

namespace tk {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace tk

static int g_fail = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);     \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

using Shape = std::vector<int64_t>;
static const int32_t* const kAddendDev = (const int32_t*)0x50000000;
static const int32_t* const kAddendHost = (const int32_t*)0x60000000;
static const tk::CaptureOptions kAll{8, true, true, true};

// A node list with made-up addresses: device buffers 256-byte aligned, records laid into an image
// in the order given to place() (default: node order), each after a 23-byte header, so at any
// alignment.
struct Net {
  std::vector<tk::Node> nodes;
  std::vector<void*> dst;
  uintptr_t dev = 0x100000;
  Net() { nodes.reserve(16); }
  static void set(tk::OwnedTensor* o, uintptr_t at, const Shape& shape, int code, int bits) {
    tk_tensor t{};
    t.data = (void*)at;
    t.ndim = (int)shape.size();
    t.shape = const_cast<int64_t*>(shape.data());
    t.dtype = {(uint8_t)code, (uint8_t)bits, 1};
    t.device = {TK_DEV_ROCM, 0};
    o->assign(&t);
  }
  tk::Node& node(int kind, int n_in, int n_out) {
    nodes.emplace_back();
    tk::Node& n = nodes.back();
    n.desc.kind = kind, n.desc.n_inputs = n_in, n.desc.n_outputs = n_out;
    for (int k = 0; k < TK_MAX_NODE_OUTPUTS; ++k) n.outp[k] = &n.out[k].t;
    return n;
  }
  uintptr_t buffer(int64_t bytes) {
    const uintptr_t at = dev;
    dev += (uintptr_t)((bytes + 255) / 256 * 256 + 256);
    return at;
  }
  void in(tk::Node& n, int k, const tk::OwnedTensor& from) { n.in[k] = from; }
  void in(tk::Node& n, int k, const Shape& s, int code, int bits) { set(&n.in[k], buffer(4096), s, code, bits); }
  void out(tk::Node& n, int k, const Shape& s, int code, int bits) {
    set(&n.out[k], 0, s, code, bits);
    n.out[k].t.data = (void*)buffer(tk::nbytes(&n.out[k].t));
  }
  // image addresses for the records in `order` (node, output); empty: all of them in node order
  void place(std::vector<std::pair<int, int>> order = {}) {
    if (order.empty())
      for (size_t i = 0; i < nodes.size(); ++i)
        for (int k = 0; k < nodes[i].desc.n_outputs; ++k) order.push_back({(int)i, k});
    dst.assign(nodes.size() * TK_MAX_NODE_OUTPUTS, nullptr);
    uintptr_t img = 0x7000000000;
    for (auto [i, k] : order) {
      img += 23;
      dst[i * TK_MAX_NODE_OUTPUTS + k] = (void*)img;
      img += (uintptr_t)tk::nbytes(&nodes[i].out[k].t);
    }
  }
};

static int plan_net(const Net& net, const tk::CaptureOptions& opt, tk::CapturePlan* p) {
  tk::g_err.clear();
  if (const int rc = tk::capture_plan_records(net.nodes, net.dst.data(), opt, p)) return rc;
  if (p->recs.empty()) return TK_OK;
  return tk::capture_plan_chunks((int)net.nodes.size(), opt.chunks, kAddendDev, kAddendHost, p);
}

static const tk::CaptureRecord* rec_of(const tk::CapturePlan& p, int node, int out) {
  for (const tk::CaptureRecord& r : p.recs)
    if (r.node == node && r.out == out) return &r;
  return nullptr;
}
// the coding of a record as one word: raw, int32 (plain), diff, bias, clamp
static std::string coding(const tk::CapturePlan& p, int node, int out) {
  const tk::CaptureRecord* r = rec_of(p, node, out);
  if (!r) return "none";
  if (!r->wire) return r->diff || r->clamp || r->bias ? "bad" : "raw";
  if (r->clamp) return r->diff || r->bias ? "bad" : "clamp";
  if (r->bias) return r->diff ? "bias" : "bad";
  return r->diff ? "diff" : "int32";
}

// Everything that holds for any plan: chunks, partition, pack table, raw ranges, segments, units.
static void check_plan(const Net& net, const tk::CaptureOptions& opt, const tk::CapturePlan& p) {
  const std::vector<tk::CaptureRecord>& recs = p.recs;
  size_t want = 0;
  for (void* d : net.dst) want += d != nullptr;
  CHECK(recs.size() == want);  // (the nets here have no empty records)
  CHECK(p.host_lo == recs.front().host && p.span == recs.back().host + recs.back().bytes - p.host_lo);
  if (!opt.wire) {
    CHECK(!p.wire && p.wchunks.empty() && p.wire_segs.empty() && p.addend_total == 0);
    for (const tk::CaptureRecord& r : recs) CHECK(!r.wire && !r.diff && !r.clamp && !r.bias);
  } else if (p.wire) {
    CHECK(p.wchunks.size() == p.chunks.size());
  }
  int64_t at = 0, addends = 0;
  size_t next_rec = 0, table_at = 0, seg_at = 0;
  int last_after = -1;
  for (size_t c = 0; c < p.chunks.size(); ++c) {
    const tk::CapturePlan::Chunk& ch = p.chunks[c];
    CHECK(ch.off == at && ch.len > 0 && ch.after_node > last_after && ch.after_node < (int)net.nodes.size());
    CHECK(ch.table_off == (int64_t)table_at);
    at += ch.len, last_after = ch.after_node;
    const tk::CapturePlan::WireChunk* wc = p.wire ? &p.wchunks[c] : nullptr;
    if (wc) CHECK(wc->seg_off == (int64_t)seg_at || wc->segs.empty());
    int64_t blocks = 0, coded_bytes = 0;
    int n_rec = 0;
    size_t range_at = 0, seg_in = 0;
    std::vector<tk_wire_record> wrecs;    // the chunk's coded records as the codec sees them
    std::vector<int> chain_of_seg;        // per segment of the chunk: length of its record's chain
    bool prev_raw = false, prev_coded = false;
    for (; next_rec < recs.size() && recs[next_rec].host - p.host_lo < at; ++next_rec) {
      const tk::CaptureRecord& r = recs[next_rec];
      const int64_t off = r.host - p.host_lo;
      CHECK(off >= ch.off && off + r.bytes <= at && r.node <= ch.after_node);
      const tk::Node& n = net.nodes[r.node];
      CHECK(r.t == &n.out[r.out].t && r.src == tk::ptr(r.t) && r.bytes == tk::nbytes(r.t));
      CHECK(r.host == (char*)net.dst[r.node * TK_MAX_NODE_OUTPUTS + r.out]);
      if (!r.wire) {
        // one pack table entry; the workgroup count restated: 16-byte mirror chunks touched, 256 each
        CHECK(table_at < p.table.size());
        const tk::PackRec& t = p.table[table_at++];
        CHECK(t.src == (const uint8_t*)r.src && t.dst == off && t.bytes == r.bytes && t.first_blk == blocks);
        const int64_t chunks16 = (off + r.bytes + 15) / 16 - off / 16;
        CHECK(tk::pack_rec_blocks(off, r.bytes) == (chunks16 + 255) / 256);
        blocks += (chunks16 + 255) / 256;
        ++n_rec;
        if (wc) {  // raw ranges: one per run of adjacent raw records, first byte to last byte
          if (!prev_raw) ++range_at;
          CHECK(range_at <= wc->raw.size());
          const tk::CapturePlan::Range& g = wc->raw[range_at - 1];
          CHECK(g.off <= off && off + r.bytes <= g.off + g.len);
          if (!prev_raw) CHECK(g.off == off);
          const bool run_ends = next_rec + 1 == recs.size() || recs[next_rec + 1].wire ||
                                recs[next_rec + 1].host - p.host_lo >= at;
          if (run_ends) CHECK(g.off + g.len == off + r.bytes);
          if (range_at > 1) CHECK(wc->raw[range_at - 2].off + wc->raw[range_at - 2].len <= g.off);
        }
        prev_raw = true, prev_coded = false;
        continue;
      }
      CHECK(wc != nullptr);
      if (!wc) continue;
      const int esize = tk::elem_bytes(r.t);
      const int64_t n_el = r.bytes / esize;
      const bool pred = r.diff || r.clamp;
      CHECK(!(r.diff && r.clamp) && (!r.bias || r.diff) && (!pred || next_rec > 0));
      const tk::CaptureRecord* pv = pred ? &recs[next_rec - 1] : nullptr;
      if (pv) CHECK(pv->bytes == r.bytes && tk::elem_bytes(pv->t) == esize);
      const bool chained = pred && prev_coded;  // the predecessor is coded in this chunk
      const int kind = esize == 4 ? tk::kWireI32 : tk::is_int(r.t, 8) ? tk::kWireI8 : tk::kWireU8;
      wrecs.push_back({0, n_el, chained, kind});
      if (r.bias) {
        CHECK(r.addend_at == addends && r.channels >= 1 && r.plane >= 1);
        addends += r.channels;
      }
      // the record's segments: consecutive, whole but the last, both sides at esize * e0
      const int64_t S = (n_el + tk::kWireSegElems - 1) / tk::kWireSegElems;
      // within a chain of k records of S segments each, record m's segments start at first + m * S
      int chain = 1;
      if (chained) chain = chain_of_seg.back() + 1;
      for (int64_t j = 0; j < S; ++j) {
        CHECK(seg_in < wc->segs.size() && seg_at < p.wire_segs.size());
        if (seg_in >= wc->segs.size() || seg_at >= p.wire_segs.size()) break;
        const tk::WireSegHost& h = wc->segs[seg_in++];
        const tk::WireSegDev& d = p.wire_segs[seg_at++];
        const int64_t e0 = j * tk::kWireSegElems;
        const int32_t sn = (int32_t)(j + 1 < S ? tk::kWireSegElems : n_el - e0);
        CHECK(h.n == sn && d.n == sn && h.kind == kind && d.kind == kind);
        CHECK(d.src == (const char*)r.src + esize * e0 && h.dst == r.host + esize * e0);
        CHECK(d.prev == (pv ? (const char*)pv->src + esize * e0 : nullptr));
        CHECK(h.prev == (pv ? pv->host + esize * e0 : nullptr));
        if (r.bias) {
          const tk::WireBias &db = d.bias, &hb = h.bias;
          CHECK(db.addend == kAddendDev + r.addend_at && hb.addend == kAddendHost + r.addend_at);
          CHECK(db.plane == r.plane && db.channels == r.channels && hb.plane == r.plane && hb.channels == r.channels);
          const int32_t c0 = (int32_t)((e0 / r.plane) % r.channels), r0 = (int32_t)(e0 % r.plane);
          CHECK(db.c0 == c0 && db.r0 == r0 && hb.c0 == c0 && hb.r0 == r0);
          const tk::WireSegPos pos = tk::wire_seg_pos(e0, r.plane, r.channels);
          CHECK(pos.c0 == c0 && pos.r0 == r0);
        } else {
          CHECK(!d.bias.addend && !h.bias.addend && !d.bias.plane && !d.bias.channels && !h.bias.plane && !h.bias.channels);
        }
        chain_of_seg.push_back(chain);
      }
      coded_bytes += r.bytes;
      prev_raw = false, prev_coded = true;
    }
    CHECK(ch.n_rec == n_rec && ch.blocks == blocks);
    if (!wc) continue;
    CHECK(range_at == wc->raw.size() && seg_in == wc->segs.size() && wc->coded_bytes == coded_bytes);
    if (wrecs.empty()) {
      CHECK(wc->units.empty() && wc->bound == 0);
      continue;
    }
    CHECK(wc->bound == tk_wire_bound(wrecs.data(), (int)wrecs.size()));
    // units: every segment once, the k-th of a unit being its chain's k-th record (so a unit
    // neither stops short of its chain's end nor runs past it)
    std::vector<int> seen(wc->segs.size(), 0);
    for (const tk::WireUnit& u : wc->units) {
      CHECK(u.count >= 1 && u.first >= 0);
      for (int k = 0; k < u.count; ++k) {
        const int64_t s = u.first + (int64_t)k * u.stride;
        CHECK(s < (int64_t)seen.size());
        if (s >= (int64_t)seen.size()) break;
        ++seen[s];
        CHECK(chain_of_seg[s] == k + 1);
        if (k) CHECK(wc->segs[s].prev == wc->segs[s - u.stride].dst);  // decoded right after its predecessor
      }
    }
    for (int s : seen) CHECK(s == 1);
  }
  CHECK(at == p.span && next_rec == recs.size() && table_at == p.table.size() && seg_at == p.wire_segs.size());
  CHECK(addends == p.addend_total);
}

// conv -> bias_add -> requantize -> clip as four nodes (records longer than one segment), a conv
// block and a dense block with their fused records, and a float tail
static Net model_net() {
  Net net;
  const Shape big{3, 24, 17, 17}, small{3, 8, 9, 9}, fc{1, 10};
  tk::Node& conv = net.node(TK_NODE_CONV2D, 2, 1);
  net.in(conv, 0, {3, 8, 19, 19}, TK_DL_INT, 8), net.in(conv, 1, {24, 8, 3, 3}, TK_DL_INT, 8);
  net.out(conv, 0, big, TK_DL_INT, 32);
  tk::Node& ba = net.node(TK_NODE_BIAS_ADD, 2, 1);
  ba.desc.attrs.bias_add.axis = -3;
  net.in(ba, 0, conv.out[0]), net.in(ba, 1, {24}, TK_DL_INT, 32);
  net.out(ba, 0, big, TK_DL_INT, 32);
  tk::Node& rq = net.node(TK_NODE_REQUANTIZE, 1, 1);
  net.in(rq, 0, ba.out[0]);
  net.out(rq, 0, big, TK_DL_INT, 8);
  tk::Node& clip = net.node(TK_NODE_CLIP, 1, 1);
  net.in(clip, 0, rq.out[0]);
  net.out(clip, 0, big, TK_DL_INT, 8);
  tk::Node& cb = net.node(TK_NODE_CONV_BLOCK, 3, 4);
  cb.desc.attrs.block.has_clip = 1;
  net.in(cb, 0, clip.out[0]), net.in(cb, 1, {8, 24, 9, 9}, TK_DL_INT, 8), net.in(cb, 2, {8}, TK_DL_INT, 32);
  net.out(cb, 0, small, TK_DL_INT, 32), net.out(cb, 1, small, TK_DL_INT, 32);
  net.out(cb, 2, small, TK_DL_INT, 8), net.out(cb, 3, small, TK_DL_INT, 8);
  tk::Node& db = net.node(TK_NODE_DENSE_BLOCK, 3, 3);
  net.in(db, 0, cb.out[3]), net.in(db, 1, {10, 1944}, TK_DL_INT, 8), net.in(db, 2, {10}, TK_DL_INT, 32);
  net.out(db, 0, fc, TK_DL_INT, 32), net.out(db, 1, fc, TK_DL_INT, 32), net.out(db, 2, fc, TK_DL_UINT, 8);
  tk::Node& deq = net.node(TK_NODE_DEQUANTIZE, 1, 1);
  net.in(deq, 0, db.out[2]);
  net.out(deq, 0, fc, TK_DL_FLOAT, 32);
  net.place();
  return net;
}

static void check_model() {
  Net net = model_net();
  for (int chunks : {1, 8, 200})
    for (int wire = 0; wire < 2; ++wire) {
      tk::CaptureOptions opt{chunks, wire != 0, true, true};
      tk::CapturePlan p;
      CHECK(plan_net(net, opt, &p) == TK_OK);
      check_plan(net, opt, p);
      CHECK(p.wire == (wire != 0));
      if (chunks == 1) CHECK(p.chunks.size() == 1 && p.chunks[0].after_node == 6);
      if (chunks == 8) CHECK(p.chunks.size() > 1 && p.chunks.size() <= 7);
      // more chunks than records: one per node, but the dense block's few bytes wait for the tail
      if (chunks == 200) CHECK(p.chunks.size() == 6 && p.chunks[4].after_node == 4 && p.chunks[5].after_node == 6);
      if (!wire) continue;
      CHECK(coding(p, 0, 0) == "int32" && coding(p, 1, 0) == "bias" && coding(p, 2, 0) == "raw" && coding(p, 3, 0) == "clamp");
      CHECK(coding(p, 4, 0) == "int32" && coding(p, 4, 1) == "bias" && coding(p, 4, 2) == "raw" && coding(p, 4, 3) == "clamp");
      CHECK(coding(p, 5, 0) == "int32" && coding(p, 5, 1) == "bias" && coding(p, 5, 2) == "raw" && coding(p, 6, 0) == "raw");
      const tk::CaptureRecord *ba = rec_of(p, 1, 0), *cb = rec_of(p, 4, 1), *db = rec_of(p, 5, 1);
      CHECK(ba->plane == 289 && ba->channels == 24 && ba->bias == &net.nodes[1].in[1].t);  // axis -3 of 4
      CHECK(cb->plane == 81 && cb->channels == 8 && cb->bias == &net.nodes[4].in[2].t);
      CHECK(db->plane == 1 && db->channels == 10 && db->bias == &net.nodes[5].in[2].t);
      CHECK(p.addend_total == 42);
      // the uint8 record of the dense block and the float record after it: one raw range
      if (chunks != 200) CHECK(p.wchunks.back().raw.back().len == 10 + 23 + 40);
      if (chunks != 200) continue;
      // The bias_add record and its convolution lie in different chunks: its two segments still
      // point at the convolution's buffer and image bytes, and nothing chains them in the decode
      // order (check_plan: prev; here: counts of 1).  The clip after the requantize likewise.
      CHECK(p.chunks[0].after_node == 0 && p.chunks[1].after_node == 1);
      const tk::CapturePlan::WireChunk& w = p.wchunks[1];
      const tk::CaptureRecord* conv = rec_of(p, 0, 0);
      CHECK(w.segs.size() == 2 && w.units.size() == 2 && w.units[0].count == 1 && w.units[1].count == 1);
      CHECK(w.segs[0].prev == conv->host && w.segs[1].prev == conv->host + 4 * tk::kWireSegElems);
      CHECK(p.wire_segs[w.seg_off].prev == conv->src && w.segs[1].bias.c0 == (tk::kWireSegElems / 289) % 24);
      CHECK(p.wchunks[3].units.size() == 2 && p.wchunks[3].units[0].count == 1 && p.wchunks[3].segs[0].prev == rec_of(p, 2, 0)->host);
      // in one chunk the same records are chained
      tk::CapturePlan one;
      CHECK(plan_net(net, {1, true, true, true}, &one) == TK_OK && one.wchunks[0].units[0].count == 2);
    }
  // records whose image order is not the node order: a chunk waits for the latest producer below its cut
  net.place({{4, 0}, {0, 0}, {5, 2}, {1, 0}, {6, 0}, {2, 0}, {4, 3}, {3, 0}, {5, 0}});
  for (int chunks : {1, 8, 200}) {
    tk::CaptureOptions opt{chunks, true, true, true};
    tk::CapturePlan p;
    CHECK(plan_net(net, opt, &p) == TK_OK);
    check_plan(net, opt, p);
    CHECK(p.chunks[0].after_node >= 4);
  }
  // no record has a destination: nothing planned, no error
  net.dst.assign(net.dst.size(), nullptr);
  tk::CapturePlan none;
  CHECK(plan_net(net, kAll, &none) == TK_OK && none.recs.empty() && none.chunks.empty());
}

// Two or three records X, Y (and Z) made by `build`, planned with `opt`: the coding of each.
template <typename F>
static std::vector<std::string> decide(F&& build, tk::CaptureOptions opt = kAll) {
  Net net;
  build(net);
  if (net.dst.empty()) net.place();
  tk::CapturePlan p;
  CHECK(plan_net(net, opt, &p) == TK_OK);
  check_plan(net, opt, p);
  std::vector<std::string> out;
  for (size_t i = 0; i < net.nodes.size(); ++i)
    for (int k = 0; k < net.nodes[i].desc.n_outputs; ++k) out.push_back(coding(p, (int)i, k));
  return out;
}
using Words = std::vector<std::string>;

static void check_decisions() {
  const Shape sh{3, 8, 9, 9};
  static int64_t strides[4] = {648, 81, 9, 1};
  // --- int32 records: coded when compact and 4-byte aligned
  auto two_i32 = [&](Net& net) {
    tk::Node& a = net.node(TK_NODE_CONV2D, 0, 1);
    net.out(a, 0, sh, TK_DL_INT, 32);
    tk::Node& b = net.node(TK_NODE_CAST, 1, 1);
    net.in(b, 0, a.out[0]);
    net.out(b, 0, sh, TK_DL_INT, 32);
  };
  CHECK((decide(two_i32) == Words{"int32", "diff"}));  // same shape, another buffer: differenced
  CHECK((decide(two_i32, {8, true, false, false}) == Words{"int32", "diff"}));
  CHECK((decide([&](Net& net) { two_i32(net), net.nodes[0].out[0].t.strides = strides; }) == Words{"raw", "int32"}));
  CHECK((decide([&](Net& net) { two_i32(net), net.nodes[0].out[0].t.byte_offset = 2; }) == Words{"raw", "int32"}));
  CHECK((decide([&](Net& net) { two_i32(net), net.nodes[1].out[0].t.strides = strides; }) == Words{"int32", "raw"}));
  CHECK((decide([&](Net& net) { two_i32(net), net.nodes[1].out[0].t.byte_offset = 2; }) == Words{"int32", "raw"}));
  // the same buffer twice (an in-place op traced under two names): coded, not differenced
  CHECK((decide([&](Net& net) { two_i32(net), net.nodes[1].out[0].t.data = net.nodes[0].out[0].t.data; }) == Words{"int32", "int32"}));
  // another shape (also with the same element count): not differenced
  CHECK((decide([&](Net& net) {
          two_i32(net);
          net.out(net.nodes[1], 0, {3, 8, 81}, TK_DL_INT, 32);
        }) == Words{"int32", "int32"}));
  CHECK((decide([&](Net& net) {
          two_i32(net);
          net.out(net.nodes[1], 0, {3, 8, 9, 8}, TK_DL_INT, 32);
        }) == Words{"int32", "int32"}));
  // after a raw record (an int8 one, or an int32 one that is not coded): not differenced
  CHECK((decide([&](Net& net) {
          two_i32(net);
          net.out(net.nodes[0], 0, sh, TK_DL_INT, 8);
        }) == Words{"raw", "int32"}));
  CHECK((decide([&](Net& net) {
          two_i32(net);
          net.out(net.nodes[0], 0, sh, TK_DL_UINT, 32);
        }) == Words{"raw", "int32"}));

  // --- bias coding: a standalone bias_add over its input
  auto bias_add = [&](Net& net, const Shape& s, int axis, const Shape& bias_shape) {
    tk::Node& a = net.node(TK_NODE_CONV2D, 0, 1);
    net.out(a, 0, s, TK_DL_INT, 32);
    tk::Node& b = net.node(TK_NODE_BIAS_ADD, 2, 1);
    b.desc.attrs.bias_add.axis = axis;
    net.in(b, 0, a.out[0]), net.in(b, 1, bias_shape, TK_DL_INT, 32);
    net.out(b, 0, s, TK_DL_INT, 32);
  };
  auto plain = [&](Net& net) { bias_add(net, sh, 1, {8}); };
  CHECK((decide(plain) == Words{"int32", "bias"}));
  CHECK((decide([&](Net& net) { bias_add(net, sh, -1, {9}); }) == Words{"int32", "bias"}));
  CHECK((decide([&](Net& net) { bias_add(net, sh, 3, {9}); }) == Words{"int32", "bias"}));
  {
    Net net;
    bias_add(net, sh, -1, {9});
    net.place();
    tk::CapturePlan p;
    CHECK(plan_net(net, kAll, &p) == TK_OK && rec_of(p, 1, 0)->plane == 1 && rec_of(p, 1, 0)->channels == 9);
    Net net0;
    bias_add(net0, sh, -4, {3});
    net0.place();
    tk::CapturePlan p0;
    CHECK(plan_net(net0, kAll, &p0) == TK_OK && rec_of(p0, 1, 0)->plane == 648 && rec_of(p0, 1, 0)->channels == 3);
  }
  // each of these leaves a plain difference
  const Words plain_diff{"int32", "diff"};
  CHECK(decide(plain, {8, true, true, false}) == plain_diff);                                    // the option
  CHECK(decide([&](Net& net) { bias_add(net, sh, 1, {9}); }) == plain_diff);                    // another length
  CHECK(decide([&](Net& net) { bias_add(net, sh, 4, {8}); }) == plain_diff);                    // axis past the rank
  CHECK(decide([&](Net& net) { bias_add(net, sh, -5, {8}); }) == plain_diff);                   // axis below it
  CHECK(decide([&](Net& net) { plain(net), net.nodes[1].in[1].t.dtype.code = TK_DL_UINT; }) == plain_diff);
  CHECK(decide([&](Net& net) { plain(net), net.nodes[1].in[1].t.dtype.bits = 16; }) == plain_diff);
  CHECK(decide([&](Net& net) { plain(net), net.nodes[1].in[1].t.dtype.code = TK_DL_FLOAT; }) == plain_diff);
  static int64_t bias_stride[1] = {2};
  CHECK(decide([&](Net& net) { plain(net), net.nodes[1].in[1].t.strides = bias_stride; }) == plain_diff);
  CHECK(decide([&](Net& net) { plain(net), net.nodes[1].in[1].t.data = nullptr; }) == plain_diff);
  CHECK(decide([&](Net& net) { plain(net), net.nodes[1].desc.n_inputs = 1; }) == plain_diff);    // no bias input
  CHECK(decide([&](Net& net) { plain(net), net.nodes[1].desc.kind = TK_NODE_CAST; }) == plain_diff);
  // the bias_add of another tensor than the record before it
  CHECK(decide([&](Net& net) { plain(net), net.nodes[1].in[0].t.data = (void*)0x999000; }) == plain_diff);
  // 2^31 elements: differenced, not bias-coded (one chunk: 2 x 131072 segments)
  CHECK(decide([&](Net& net) { bias_add(net, {2, (int64_t)1 << 30}, 0, {2}); }, {1, true, true, true}) == plain_diff);
  // after a raw predecessor there is no difference to take the bias from
  CHECK((decide([&](Net& net) { plain(net), net.nodes[0].out[0].t.byte_offset = 2; }) == Words{"raw", "int32"}));

  // --- bias coding inside blocks: output 1 over output 0, bias in input 2
  auto block = [&](Net& net, int kind, const Shape& s, const Shape& bias_shape, int n_out, bool has_clip) {
    tk::Node& b = net.node(kind, 3, n_out);
    b.desc.attrs.block.has_clip = has_clip;
    net.in(b, 2, bias_shape, TK_DL_INT, 32);
    net.out(b, 0, s, TK_DL_INT, 32), net.out(b, 1, s, TK_DL_INT, 32);
    for (int k = 2; k < n_out; ++k) net.out(b, k, s, TK_DL_INT, 8);
  };
  CHECK((decide([&](Net& net) { block(net, TK_NODE_CONV_BLOCK, sh, {8}, 4, true); }) == Words{"int32", "bias", "raw", "clamp"}));
  CHECK((decide([&](Net& net) { block(net, TK_NODE_DENSE_BLOCK, {3, 10}, {10}, 4, true); }) == Words{"int32", "bias", "raw", "clamp"}));
  CHECK((decide([&](Net& net) { block(net, TK_NODE_DENSE_BLOCK, {3, 10}, {3}, 3, false); }) == Words{"int32", "diff", "raw"}));
  CHECK((decide([&](Net& net) { block(net, TK_NODE_CONV_BLOCK, sh, {8}, 3, false), net.nodes[0].desc.n_inputs = 2; }) ==
         Words{"int32", "diff", "raw"}));
  // output 1 placed before output 0 in the image: no predecessor to add the bias to
  CHECK((decide([&](Net& net) {
          block(net, TK_NODE_CONV_BLOCK, sh, {8}, 2, false);
          net.place({{0, 1}, {0, 0}});
        }) == Words{"diff", "int32"}));

  // --- clamp coding
  // the last output of a block with has_clip over the output before it; without the flag, raw
  CHECK((decide([&](Net& net) { block(net, TK_NODE_CONV_BLOCK, sh, {8}, 4, false); }) == Words{"int32", "bias", "raw", "raw"}));
  CHECK((decide([&](Net& net) { block(net, TK_NODE_CONV_BLOCK, sh, {8}, 5, true); }) == Words{"int32", "bias", "raw", "raw", "clamp"}));
  CHECK((decide([&](Net& net) { block(net, TK_NODE_CONV_BLOCK, sh, {8}, 4, true); }, {8, true, false, true}) ==
         Words{"int32", "bias", "raw", "raw"}));  // the option
  auto add_block = [&](Net& net, int clip_code) {
    tk::Node& b = net.node(TK_NODE_ADD_BLOCK, 2, 2);
    b.desc.attrs.add_block.has_clip = 1;
    net.out(b, 0, sh, TK_DL_INT, 8), net.out(b, 1, sh, clip_code, 8);
  };
  CHECK((decide([&](Net& net) { add_block(net, TK_DL_INT); }) == Words{"raw", "clamp"}));
  CHECK((decide([&](Net& net) { add_block(net, TK_DL_UINT); }) == Words{"raw", "raw"}));  // another dtype
  CHECK((decide([&](Net& net) { add_block(net, TK_DL_INT), net.nodes[0].desc.attrs.add_block.has_clip = 0; }) == Words{"raw", "raw"}));
  CHECK((decide([&](Net& net) { add_block(net, TK_DL_INT), net.out(net.nodes[0], 1, {3, 8, 81}, TK_DL_INT, 8); }) == Words{"raw", "raw"}));
  CHECK((decide([&](Net& net) { add_block(net, TK_DL_INT), net.nodes[0].out[1].t.strides = strides; }) == Words{"raw", "raw"}));
  CHECK((decide([&](Net& net) { add_block(net, TK_DL_INT), net.nodes[0].out[0].t.strides = strides; }) == Words{"raw", "raw"}));
  // a TK_NODE_CLIP over the record before it, uint8 too; a clip of a clip chains
  auto clips = [&](Net& net, int code, int n_clips) {
    tk::Node& a = net.node(TK_NODE_REQUANTIZE, 0, 1);
    net.out(a, 0, sh, code, 8);
    for (int k = 0; k < n_clips; ++k) {
      tk::Node& c = net.node(TK_NODE_CLIP, 1, 1);
      net.in(c, 0, net.nodes[k].out[0]);
      net.out(c, 0, sh, code, 8);
    }
  };
  CHECK((decide([&](Net& net) { clips(net, TK_DL_INT, 1); }) == Words{"raw", "clamp"}));
  CHECK((decide([&](Net& net) { clips(net, TK_DL_UINT, 2); }) == Words{"raw", "clamp", "clamp"}));
  CHECK((decide([&](Net& net) { clips(net, TK_DL_INT, 1); }, {8, true, false, true}) == Words{"raw", "raw"}));
  CHECK((decide([&](Net& net) { clips(net, TK_DL_INT, 1), net.nodes[1].out[0].t.dtype.code = TK_DL_UINT; }) == Words{"raw", "raw"}));
  // the predecessor in the image is not the declared input: the clip of another tensor, another
  // record in between, or a node that declares no clip
  CHECK((decide([&](Net& net) { clips(net, TK_DL_INT, 1), net.nodes[1].in[0].t.data = (void*)0x999000; }) == Words{"raw", "raw"}));
  CHECK((decide([&](Net& net) { clips(net, TK_DL_INT, 2), net.in(net.nodes[2], 0, net.nodes[0].out[0]); }) == Words{"raw", "clamp", "raw"}));
  CHECK((decide([&](Net& net) { clips(net, TK_DL_INT, 1), net.nodes[1].desc.kind = TK_NODE_CAST; }) == Words{"raw", "raw"}));
  CHECK((decide([&](Net& net) { clips(net, TK_DL_INT, 1), net.nodes[1].out[0].t.data = net.nodes[0].out[0].t.data; }) == Words{"raw", "raw"}));
  // only 1-byte clips are clamp-coded: an int32 clip is a plain difference
  CHECK((decide([&](Net& net) {
          clips(net, TK_DL_INT, 1);
          net.out(net.nodes[0], 0, sh, TK_DL_INT, 32), net.out(net.nodes[1], 0, sh, TK_DL_INT, 32);
          net.in(net.nodes[1], 0, net.nodes[0].out[0]);
        }) == Words{"int32", "diff"}));
}

static void check_refusals() {
  Net net = model_net();
  // the bias_add record starts inside the convolution's
  net.dst[1 * TK_MAX_NODE_OUTPUTS] = (char*)net.dst[0] + 100;
  tk::CapturePlan p;
  CHECK(plan_net(net, kAll, &p) == TK_ERR_INVALID_ARG);
  CHECK(tk::g_err == "tk_module_run_graph: overlapping record destinations");
  // the same destination twice
  net = model_net();
  net.dst[1 * TK_MAX_NODE_OUTPUTS] = net.dst[0];
  tk::CapturePlan q;
  CHECK(plan_net(net, {1, false, true, true}, &q) == TK_ERR_INVALID_ARG);
  CHECK(tk::g_err == "tk_module_run_graph: overlapping record destinations");
  // touching records are fine
  net = model_net();
  net.dst[1 * TK_MAX_NODE_OUTPUTS] = (char*)net.dst[0] + tk::nbytes(&net.nodes[0].out[0].t);
  tk::CapturePlan r;
  CHECK(plan_net(net, kAll, &r) == TK_OK && tk::g_err.empty());
}

int main() {
  check_model();
  check_decisions();
  check_refusals();
  std::printf(g_fail ? "capture_plan_check: %d failures\n" : "capture_plan_check: ok\n", g_fail);
  return g_fail ? 1 : 0;
}
