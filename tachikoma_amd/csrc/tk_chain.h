// The chain check (tk_chain.hip): the tail ops of fused nodes, each recomputed from its own recorded
// input and compared with its recorded output.  Shared by the kernel file and by tk_runtime.cc,
// which lays the table of a module out once and keeps it on the device.
#pragma once

#include <string>
#include <vector>

#include "tk_common.h"

namespace tk {

// Elements one lane takes per step (16 bytes of an int32 record, a 4-byte run of a 1-byte one) and
// elements one workgroup takes (kChainSteps steps of 256 lanes).
constexpr int kChainVec = 4;
constexpr int kChainSteps = 4;
constexpr int kChainTile = 256 * kChainVec * kChainSteps;

// tail ops in chain order; a chain's report entries follow it
enum ChainOp : int32_t { kChainBias = 0, kChainRequantize = 1, kChainAdd = 2, kChainClip = 3, kChainOps = 4 };

// One fused chain as the kernel sees it.  conv -> bias_add -> requantize -> [qnn.add] -> [clip]
// (has_i32) or, for an add block, add -> clip (no int32 part: `rq` is then the add record).
struct ChainDev {
  const int32_t* conv;
  const int32_t* bias_out;
  const int32_t* bias;   // [C]
  const uint8_t* rq;     // the requantize record (the clip's predecessor when !has_add)
  const uint8_t* res;    // the other qnn.add operand
  const uint8_t* add;
  const uint8_t* clip;
  RqParams rq_p;         // the node's requantize; qmin / qmax: the 8-bit dtype's range
  RqParams add_pb, add_pr;  // RequantizeOrUpcast of the block's side and of the residual's
  int32_t add_up_b, add_up_r, add_zp;
  int32_t clip_lo, clip_hi;
  int32_t has_i32, has_add, has_clip, is_u8;
  int32_t vec;           // every record allows the wide loads (int32: 16-byte, 1-byte: 4-byte aligned)
  int32_t C, HW;         // channel of flat element e: (e / HW) % C
  int64_t n;             // elements of each record
  int64_t first_blk;     // first workgroup of this chain in the launch
  int32_t rep[kChainOps];  // report entry of each tail op, -1: the chain has none
};

// A chain described by tensors, before it is laid out.  outs: the node's records in chain order.
struct ChainSpec {
  int kind;  // TK_NODE_CONV_BLOCK / TK_NODE_DENSE_BLOCK / TK_NODE_ADD_BLOCK
  const tk_tensor* const* outs;
  int n_outs;
  const tk_tensor* bias;
  const tk_tensor* residual;
  const tk_block_attrs* block;          // conv / dense blocks
  const tk_add_block_attrs* add_block;  // add blocks
};

// Validates `spec` under the entry point's name `who` and appends its chain to `table` (a chain
// of one record appends nothing); report entries are numbered from *n_report on, workgroups from
// *blocks on.  Host only.
int chain_append(const ChainSpec& spec, const char* who, std::vector<ChainDev>* table, int* n_report, int64_t* blocks);
// Resets `report` (device, n_report entries) and checks the chains of `table` (device) on `s`.
int chain_check_impl(const ChainDev* table, int n_chains, int64_t blocks, tk_wire_mismatch* report, int n_report,
                     hipStream_t s);

}  // namespace tk
