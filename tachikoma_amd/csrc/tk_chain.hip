// The chain check, for gfx950: the verdict of every tail op of a fused node from its own recorded
// input.  A conv, dense or add block is one kernel that writes its whole chain of records
// (conv -> bias_add -> requantize -> [qnn.add] -> [clip]), so a node replay can only say that the
// node differs.  When a trace file's records lie in the module's buffers every tail op is
// elementwise over records that are all there: bias_add of the conv record, requantize of the
// bias_add record, qnn.add of the requantize record and the residual, clip of its predecessor.
// This kernel computes each of them with the fused epilogues' own device functions (rq_apply and
// the qms_* forms of tk_common.h, the 256-entry RequantizeOrUpcast tables of tk_block_tail.h) and
// compares with the recorded output.  It stores nothing into a record.
//
// One launch takes every chain of a table.  A workgroup finds its chain by binary search over the
// chains' first workgroups and takes kChainTile consecutive elements of it, in kChainSteps steps of
// 256 lanes x kChainVec elements: a lane reads 16 bytes of each int32 record and the matching
// 4-byte run of each 1-byte record, every record once (the bias_add record serves as the
// bias_add's output and as the requantize's input, and so on down the chain).  The element-by-
// element path serves a chain's ragged end and chains whose buffers do not allow the wide loads.
// The channel of an element is (e / HW) % C: one 64-bit division per workgroup gives the tile's
// first row and pixel, a lane adds its 32-bit offset, and where a lane's four elements cross the
// end of a plane (H*W not a multiple of four) the later ones take the next channel's constants.
// Element offsets are 64-bit.  Counts are reduced in the workgroup and reported as the wire
// decoder's compare mode does (wire_report_mismatches): a workgroup that found a difference issues
// one atomicAdd and one 64-bit atomicMin per record, an equal chain none.  No workgroup waits for
// another.
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "tk_block_tail.h"
#include "tk_chain.h"
#include "tk_wire.h"

namespace tk {

namespace {

__device__ __forceinline__ int32_t chain_byte(uint32_t w, int j, bool is_u8) {
  const uint32_t b = (w >> (8 * j)) & 0xFFu;
  return is_u8 ? (int32_t)b : (int32_t)(int8_t)(uint8_t)b;
}

__device__ __forceinline__ int32_t chain_clamp(int32_t x, int32_t lo, int32_t hi) { return min(max(x, lo), hi); }

__global__ __launch_bounds__(256) void chain_check_kernel(const ChainDev* __restrict__ table, int n_chains,
                                                          tk_wire_mismatch* report) {
  __shared__ uint32_t s_any[4];
  __shared__ unsigned long long s_red[8];
  __shared__ int32_t lut[512];  // RequantizeOrUpcast of every 8-bit value: the block's side, the residual's
  int lo = 0, hi = n_chains - 1;
  const int64_t blk = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].first_blk <= blk) lo = mid;
    else hi = mid - 1;
  }
  const ChainDev& ch = table[lo];
  const int tid = threadIdx.x;
  const bool is_u8 = ch.is_u8, has_i32 = ch.has_i32, has_add = ch.has_add, has_clip = ch.has_clip;
  const int32_t qmin = is_u8 ? 0 : -128, qmax = is_u8 ? 255 : 127;
  if (has_add) {
    block_join_lut(tid, lut, is_u8, ch.add_up_b, ch.add_up_r, ch.add_pb, ch.add_pr);
    __syncthreads();
  }
  const int64_t n = ch.n;
  const int64_t base = (blk - ch.first_blk) * kChainTile;
  const uint32_t C = (uint32_t)ch.C, HW = (uint32_t)ch.HW;
  // the tile's first row (image x channel) and pixel: the only 64-bit division
  const int64_t row0 = base / HW;
  const uint32_t p0 = (uint32_t)(base - row0 * HW);
  const uint32_t c0 = (uint32_t)(row0 % C);
  const int32_t add_zp = ch.add_zp, clip_lo = ch.clip_lo, clip_hi = ch.clip_hi;

  uint32_t cnt[kChainOps] = {0, 0, 0, 0};
  uint32_t first[kChainOps] = {~0u, ~0u, ~0u, ~0u};  // offset in the tile of the lowest mismatch
#pragma unroll
  for (int step = 0; step < kChainSteps; ++step) {
    const uint32_t o = (uint32_t)(step * 256 + tid) * kChainVec;
    const int64_t e0 = base + o;
    if (e0 >= n) continue;
    const int valid = (int)min((int64_t)kChainVec, n - e0);
    // records of this lane's elements: conv and bias_add as int32, the 1-byte ones packed in a dword
    int32_t vc[kChainVec] = {}, vb[kChainVec] = {};
    uint32_t wq = 0, wr = 0, wa = 0, wk = 0;
    if (valid == kChainVec && ch.vec) {
      if (has_i32) {
        const tk_v4i a = __builtin_nontemporal_load(reinterpret_cast<const tk_v4i*>(ch.conv + e0));
        const tk_v4i b = __builtin_nontemporal_load(reinterpret_cast<const tk_v4i*>(ch.bias_out + e0));
        vc[0] = a.x, vc[1] = a.y, vc[2] = a.z, vc[3] = a.w;
        vb[0] = b.x, vb[1] = b.y, vb[2] = b.z, vb[3] = b.w;
      }
      wq = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(ch.rq + e0));
      if (has_add) {
        wr = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(ch.res + e0));
        wa = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(ch.add + e0));
      }
      if (has_clip) wk = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(ch.clip + e0));
    } else {
#pragma unroll
      for (int j = 0; j < kChainVec; ++j) {
        if (j >= valid) continue;
        if (has_i32) vc[j] = ch.conv[e0 + j], vb[j] = ch.bias_out[e0 + j];
        wq |= (uint32_t)ch.rq[e0 + j] << (8 * j);
        if (has_add) wr |= (uint32_t)ch.res[e0 + j] << (8 * j), wa |= (uint32_t)ch.add[e0 + j] << (8 * j);
        if (has_clip) wk |= (uint32_t)ch.clip[e0 + j] << (8 * j);
      }
    }
    // channel of element 0, then of the others
    const uint32_t x = p0 + o;
    const uint32_t dr = x / HW;
    const uint32_t p = x - dr * HW;
    const uint32_t c = (c0 + dr) % C;
    uint32_t bad[kChainOps] = {0, 0, 0, 0};  // bit j: element j differs
#pragma unroll
    for (int j = kChainVec - 1; j >= 0; --j) {
      if (j >= valid) continue;
      const int32_t q = chain_byte(wq, j, is_u8);
      if (has_i32) {
        uint32_t cj = c;
        if (p + j >= HW) {
          // past the end of the plane: one channel on when planes hold four pixels or more
          if (HW >= (uint32_t)kChainVec) cj = c + 1 == C ? 0 : c + 1;
          else cj = (c0 + (x + j) / HW) % C;
        }
        const int32_t want_b = (int32_t)((uint32_t)vc[j] + (uint32_t)ch.bias[cj]);
        bad[kChainBias] |= (uint32_t)(want_b != vb[j]) << j;
        const int32_t want_q = chain_clamp(rq_apply(vb[j], (int)cj, ch.rq_p), qmin, qmax);
        bad[kChainRequantize] |= (uint32_t)(want_q != q) << j;
      }
      int32_t pred = q;
      if (has_add) {
        // qnn.add (src/relay/qnn/op/add.cc:40-96): RQ(block) + RQ(residual) - zp_out, saturated
        const int32_t a = chain_byte(wa, j, is_u8);
        const int32_t want_a = chain_clamp(
            (int32_t)((uint32_t)lut[(wq >> (8 * j)) & 0xFFu] + (uint32_t)lut[256 + ((wr >> (8 * j)) & 0xFFu)] - (uint32_t)add_zp),
            qmin, qmax);
        bad[kChainAdd] |= (uint32_t)(want_a != a) << j;
        pred = a;
      }
      if (has_clip) bad[kChainClip] |= (uint32_t)(chain_clamp(pred, clip_lo, clip_hi) != chain_byte(wk, j, is_u8)) << j;
    }
#pragma unroll
    for (int k = 0; k < kChainOps; ++k)
      if (bad[k]) {
        cnt[k] += __builtin_popcount(bad[k]);
        first[k] = min(first[k], o + (uint32_t)__builtin_ctz(bad[k]));
      }
  }
#pragma unroll
  for (int k = 0; k < kChainOps; ++k) {
    const int r = ch.rep[k];
    if (r >= 0)  // the same for the whole workgroup
      wire_report_mismatches(cnt[k], first[k] == ~0u ? ~0ull : (unsigned long long)(base + first[k]), report + r, s_any,
                             s_red);
  }
}

RqParams chain_rq(const tk_requantize_attrs& a, int channels, bool per_axis) {
  RqParams p{};
  p.mode = a.mode;
  p.multiplier = a.multiplier;
  p.shift = a.shift;
  p.zp_in = a.input_zero_point;
  p.zp_out = a.output_zero_point;
  if (per_axis) p.ms = a.multipliers, p.ss = a.shifts, p.zps = a.input_zero_points;
  p.inner = 1;
  p.C = channels;
  return p;
}

bool same_shape(const tk_tensor* a, const tk_tensor* b) {
  if (a->ndim != b->ndim) return false;
  for (int i = 0; i < a->ndim; ++i)
    if (a->shape[i] != b->shape[i]) return false;
  return true;
}

}  // namespace

int chain_append(const ChainSpec& sp, const char* who, std::vector<ChainDev>* table, int* n_report, int64_t* blocks) {
  auto fail = [&](const std::string& msg) {
    set_error(std::string(who) + ": " + msg);
    return TK_ERR_INVALID_ARG;
  };
  const bool add_block = sp.kind == TK_NODE_ADD_BLOCK;
  if (sp.kind != TK_NODE_CONV_BLOCK && sp.kind != TK_NODE_DENSE_BLOCK && !add_block)
    return fail("a chain is a conv block, a dense block or an add block");
  if (!sp.outs || sp.n_outs < 1) return fail("null argument");
  for (int k = 0; k < sp.n_outs; ++k) {
    const tk_tensor* t = sp.outs[k];
    if (!t || (numel(t) > 0 && !t->data) || (t->ndim > 0 && !t->shape)) return fail("null record");
    if (!compact(t)) return fail("compact tensors only");
    if (!same_shape(t, sp.outs[0])) return fail("the records of a chain have one shape");
  }
  const tk_tensor* t0 = sp.outs[0];
  if (t0->ndim < 2) return fail("records need a channel axis (axis 1)");
  ChainDev ch{};
  for (int k = 0; k < kChainOps; ++k) ch.rep[k] = -1;
  int64_t hw = 1;
  for (int i = 2; i < t0->ndim; ++i) hw *= t0->shape[i];
  ch.n = numel(t0);
  if (t0->shape[1] > INT32_MAX || hw > INT32_MAX - kChainTile) return fail("tensor too large");
  ch.C = (int32_t)t0->shape[1];
  ch.HW = (int32_t)hw;
  const tk_tensor* last8 = nullptr;  // the clip's predecessor
  int n_tail = 0;
  uintptr_t align32 = 0, align8 = 0;
  if (add_block) {
    const tk_add_block_attrs* at = sp.add_block;
    if (!at) return fail("null argument");
    if (sp.n_outs != 1 + (at->has_clip ? 1 : 0)) return fail("outs = {add, [clip]}");
    if (!is_int8ish(t0)) return fail("qnn.add block: 8-bit records");
    ch.is_u8 = is_uint(t0, 8);
    ch.rq = (const uint8_t*)ptr(t0);
    last8 = t0;
    ch.has_clip = at->has_clip ? 1 : 0;
    ch.clip_lo = 0, ch.clip_hi = 0;
    if (ch.has_clip) {
      const int64_t lo = ch.is_u8 ? 0 : -128, hi = ch.is_u8 ? 255 : 127;
      ch.clip_lo = (int32_t)std::max<int64_t>(at->clip_min, lo);
      ch.clip_hi = (int32_t)std::max<int64_t>(std::min<int64_t>(at->clip_max, hi), ch.clip_lo);
    }
  } else {
    const tk_block_attrs* at = sp.block;
    if (!at || !sp.bias) return fail("null argument");
    const int has_add = at->has_add ? 1 : 0, has_clip = at->has_clip ? 1 : 0;
    if (sp.n_outs != 3 + has_add + has_clip) return fail("outs = {conv, bias_add, requantize, [add], [clip]}");
    const tk_tensor* bo = sp.outs[1];
    const tk_tensor* rq = sp.outs[2];
    if (!is_int(t0, 32) || !is_int(bo, 32)) return fail("the conv and bias_add records are int32");
    if (!is_int8ish(rq)) return fail("the requantize record is int8 / uint8");
    if (!sp.bias->data || !compact(sp.bias) || !is_int(sp.bias, 32) || numel(sp.bias) != ch.C)
      return fail("bias must be int32 [channels]");
    const tk_requantize_attrs& r = at->requantize;
    if (r.mode < TK_RQ_IDENTITY || r.mode > TK_RQ_AXIS_TONEAREST) return fail("unknown requantize mode");
    const bool per_axis = r.mode == TK_RQ_AXIS_UPWARD || r.mode == TK_RQ_AXIS_TONEAREST;
    if (per_axis && (!r.multipliers || !r.shifts)) return fail("per-axis requantize needs device multipliers / shifts");
    if (r.axis != 1 && per_axis) return fail("requantize must run along the channel axis");
    ch.has_i32 = 1;
    ch.is_u8 = is_uint(rq, 8);
    ch.conv = (const int32_t*)ptr(t0);
    ch.bias_out = (const int32_t*)ptr(bo);
    ch.bias = (const int32_t*)ptr(sp.bias);
    ch.rq = (const uint8_t*)ptr(rq);
    ch.rq_p = chain_rq(r, ch.C, true);
    if (!per_axis) ch.rq_p.ms = ch.rq_p.ss = nullptr;
    align32 = (uintptr_t)ch.conv | (uintptr_t)ch.bias_out;
    if (((uintptr_t)ch.conv | (uintptr_t)ch.bias_out | (uintptr_t)ch.bias) & 3) return fail("int32 buffers must be 4-byte aligned");
    last8 = rq;
    for (int k = 3; k < sp.n_outs; ++k)
      if (dt_of(sp.outs[k]) != dt_of(rq)) return fail("add / clip records must have the requantize record's dtype");
    if (has_add) {
      const tk_tensor* res = sp.residual;
      if (!res || !res->data || !compact(res) || dt_of(res) != dt_of(rq) || numel(res) != ch.n)
        return fail("residual must match the requantize record (same size and dtype)");
      if (at->add.lhs.mode < 0 || at->add.rhs.mode < 0 || at->add.lhs.mode > TK_RQ_TENSOR_TONEAREST ||
          at->add.rhs.mode > TK_RQ_TENSOR_TONEAREST)
        return fail("qnn.add: per-tensor parameters only");
      ch.has_add = 1;
      ch.res = (const uint8_t*)ptr(res);
      ch.add = (const uint8_t*)ptr(sp.outs[3]);
      ch.add_pb = chain_rq(at->block_is_rhs ? at->add.rhs : at->add.lhs, 1, false);
      ch.add_pr = chain_rq(at->block_is_rhs ? at->add.lhs : at->add.rhs, 1, false);
      ch.add_up_b = at->block_is_rhs ? at->add.rhs_upcast : at->add.lhs_upcast;
      ch.add_up_r = at->block_is_rhs ? at->add.lhs_upcast : at->add.rhs_upcast;
      ch.add_zp = at->add.output_zero_point;
      align8 |= (uintptr_t)ch.res | (uintptr_t)ch.add;
      last8 = sp.outs[3];
    }
    ch.has_clip = has_clip;
    if (has_clip) {
      // as the fused epilogues set them (max(min(x, a_max), a_min): a_min wins)
      const int64_t lo = ch.is_u8 ? 0 : -128, hi = ch.is_u8 ? 255 : 127;
      ch.clip_lo = (int32_t)std::max<int64_t>(at->clip_min, lo);
      ch.clip_hi = (int32_t)std::max<int64_t>(std::min<int64_t>(at->clip_max, hi), ch.clip_lo);
    }
    ch.rep[kChainBias] = (*n_report)++;
    ch.rep[kChainRequantize] = (*n_report)++;
    if (has_add) ch.rep[kChainAdd] = (*n_report)++;
    n_tail = 2 + has_add;
  }
  if (ch.has_clip) {
    const tk_tensor* cl = sp.outs[sp.n_outs - 1];
    if (dt_of(cl) != dt_of(last8)) return fail("the clip record must have its predecessor's dtype");
    ch.clip = (const uint8_t*)ptr(cl);
    align8 |= (uintptr_t)ch.clip;
    ch.rep[kChainClip] = (*n_report)++;
    ++n_tail;
  }
  align8 |= (uintptr_t)ch.rq;
  ch.vec = (align32 & 15) == 0 && (align8 & 3) == 0;
  // a single record is the head op alone; the entries of a chain of no elements stay "equal"
  if (n_tail == 0 || ch.n == 0) return TK_OK;
  ch.first_blk = *blocks;
  *blocks += (ch.n + kChainTile - 1) / kChainTile;
  table->push_back(ch);
  return TK_OK;
}

int chain_check_impl(const ChainDev* table, int n_chains, int64_t blocks, tk_wire_mismatch* report, int n_report,
                     hipStream_t s) {
  TK_CHECK_ARG(table && report && n_chains > 0 && n_report > 0 && blocks >= 0 && blocks < ((int64_t)1 << 31),
               "bad arguments");
  if (const int rc = wire_report_init(report, n_report, s)) return rc;
  if (blocks == 0) return TK_OK;
  hipLaunchKernelGGL(chain_check_kernel, dim3((unsigned)blocks), dim3(256), 0, s, table, n_chains, report);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

}  // namespace tk

extern "C" {

int tk_chain_check_tile(void) { return tk::kChainTile; }

int tk_check_chain(int kind, const tk_tensor* const* records, int n_records, const tk_tensor* bias, const void* attrs,
                   tk_wire_mismatch* report, int capacity, void* stream) {
  if (!records || !attrs || !report) {
    tk::set_error("tk_check_chain: null argument");
    return TK_ERR_INVALID_ARG;
  }
  tk::ChainSpec sp{};
  sp.kind = kind;
  sp.outs = records;
  sp.n_outs = n_records;
  sp.bias = bias;
  if (kind == TK_NODE_ADD_BLOCK) {
    sp.add_block = (const tk_add_block_attrs*)attrs;
  } else {
    sp.block = (const tk_block_attrs*)attrs;
    sp.residual = sp.block->residual;
  }
  std::vector<tk::ChainDev> table;
  int n_report = 0;
  int64_t blocks = 0;
  if (const int rc = tk::chain_append(sp, "tk_check_chain", &table, &n_report, &blocks)) return rc;
  if (n_report > capacity) {
    tk::set_error("tk_check_chain: the report holds " + std::to_string(capacity) + " entries, the chain has " +
                  std::to_string(n_report) + " tail ops");
    return TK_ERR_INVALID_ARG;
  }
  for (int i = 0; i < n_report; ++i) report[i].mismatches = 0, report[i].first = ~(uint64_t)0;
  if (table.empty()) return n_report;  // one record, or records of no elements
  hipStream_t s = tk::as_stream(stream);
  const int64_t table_bytes = tk::wire_align((int64_t)sizeof(tk::ChainDev), 64);
  void* dev = nullptr;
  TK_HIP(hipMalloc(&dev, (size_t)(table_bytes + n_report * (int64_t)sizeof(tk_wire_mismatch))));
  tk_wire_mismatch* rep = (tk_wire_mismatch*)((char*)dev + table_bytes);
  int rc = TK_OK;
  if (hipMemcpyAsync(dev, table.data(), sizeof(tk::ChainDev), hipMemcpyHostToDevice, s) != hipSuccess) {
    tk::set_error("tk_check_chain: loading the chain table failed");
    rc = TK_ERR_HIP;
  }
  if (rc == TK_OK) rc = tk::chain_check_impl((const tk::ChainDev*)dev, 1, blocks, rep, n_report, s);
  if (rc == TK_OK &&
      hipMemcpyAsync(report, rep, (size_t)n_report * sizeof(tk_wire_mismatch), hipMemcpyDeviceToHost, s) != hipSuccess) {
    tk::set_error("tk_check_chain: reading the report failed");
    rc = TK_ERR_HIP;
  }
  // the report is filled once the call's own work on `stream` is complete, as tk_compare_device_batch's
  if (hipStreamSynchronize(s) != hipSuccess && rc == TK_OK) {
    tk::set_error("tk_check_chain: the chain-check kernel failed");
    rc = TK_ERR_HIP;
  }
  (void)hipFree(dev);
  return rc == TK_OK ? n_report : rc;
}

}  // extern "C"
