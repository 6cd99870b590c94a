// Stand-alone check of the chain check's host side (tk::chain_append, csrc/tk_chain.hip) for
// sanitizer builds: the table a module's fused chains are laid out into -- report entries, first
// workgroups, the wide-load flag, the epilogue constants -- and every refusal, on tensor
// descriptors whose data pointers are never dereferenced.  CPU only; launches nothing and never
// needs a device.
//
//   hipcc -std=c++20 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=all -I include tools/chain_table_check.cc \
//       tachikoma_amd/csrc/tk_chain.hip -o chain_table_check && ./chain_table_check
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../tachikoma_amd/csrc/tk_chain.h"

namespace tk {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int wire_report_init(tk_wire_mismatch*, int, hipStream_t) { return TK_OK; }  // (tk_trace.hip; not called here)
}  // namespace tk

static int g_fail = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);     \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

struct Tensor {
  tk_tensor t{};
  std::vector<int64_t> shape;
  Tensor(uintptr_t at, std::vector<int64_t> s, int code, int bits) : shape(std::move(s)) {
    t.data = (void*)at;
    t.ndim = (int)shape.size();
    t.shape = shape.data();
    t.dtype = {(uint8_t)code, (uint8_t)bits, 1};
    t.device = {TK_DEV_ROCM, 0};
  }
};

int main() {
  const std::vector<int64_t> shape{3, 24, 9, 9};  // 5832 elements: two workgroups
  Tensor conv(0x1000, shape, TK_DL_INT, 32), bo(0x9000, shape, TK_DL_INT, 32), rq(0x11000, shape, TK_DL_INT, 8);
  Tensor add(0x13000, shape, TK_DL_INT, 8), clip(0x15000, shape, TK_DL_INT, 8), res(0x17000, shape, TK_DL_INT, 8);
  Tensor bias(0x19000, {24}, TK_DL_INT, 32);
  const tk_tensor* outs[5] = {&conv.t, &bo.t, &rq.t, &add.t, &clip.t};
  tk_block_attrs at{};
  at.requantize.mode = TK_RQ_TENSOR_UPWARD;
  at.requantize.axis = 1;
  at.requantize.multiplier = 1 << 30;
  at.requantize.shift = -7;
  at.has_clip = 1, at.clip_min = -300, at.clip_max = 100;
  at.has_add = 1, at.block_is_rhs = 1;
  at.add.lhs.mode = TK_RQ_TENSOR_UPWARD, at.add.lhs.multiplier = 11, at.add.rhs.mode = TK_RQ_IDENTITY;
  at.add.lhs_upcast = 0, at.add.rhs_upcast = 1, at.add.output_zero_point = 5;
  tk::ChainSpec sp{TK_NODE_CONV_BLOCK, outs, 5, &bias.t, &res.t, &at, nullptr};

  std::vector<tk::ChainDev> table;
  int n_report = 0;
  int64_t blocks = 0;
  CHECK(tk::chain_append(sp, "check", &table, &n_report, &blocks) == TK_OK);
  CHECK(table.size() == 1 && n_report == 4 && blocks == 2);
  {
    const tk::ChainDev& c = table[0];
    CHECK(c.rep[0] == 0 && c.rep[1] == 1 && c.rep[2] == 2 && c.rep[3] == 3 && c.first_blk == 0);
    CHECK(c.n == 5832 && c.C == 24 && c.HW == 81 && c.vec == 1 && c.has_i32 && c.has_add && c.has_clip && !c.is_u8);
    CHECK(c.clip_lo == -128 && c.clip_hi == 100);  // bounds cast to the dtype
    // the block is the rhs operand: its side takes rhs' plan, the residual lhs'
    CHECK(c.add_pb.mode == TK_RQ_IDENTITY && c.add_up_b == 1 && c.add_pr.multiplier == 11 && c.add_up_r == 0 && c.add_zp == 5);
    CHECK(c.rq_p.ms == nullptr && c.rq_p.multiplier == (1 << 30) && c.rq_p.shift == -7);
  }
  // a second chain: no add, no clip, uint8, a byte record at an odd address: narrow loads
  Tensor rq8(0x21001, {3, 10}, TK_DL_UINT, 8), c2(0x22000, {3, 10}, TK_DL_INT, 32), b2(0x23000, {3, 10}, TK_DL_INT, 32);
  Tensor bias2(0x24000, {10}, TK_DL_INT, 32);
  const tk_tensor* outs2[3] = {&c2.t, &b2.t, &rq8.t};
  tk_block_attrs at2{};
  at2.requantize.mode = TK_RQ_IDENTITY;
  tk::ChainSpec sp2{TK_NODE_DENSE_BLOCK, outs2, 3, &bias2.t, nullptr, &at2, nullptr};
  CHECK(tk::chain_append(sp2, "check", &table, &n_report, &blocks) == TK_OK);
  CHECK(table.size() == 2 && n_report == 6 && blocks == 3);
  CHECK(table[1].first_blk == 2 && table[1].rep[0] == 4 && table[1].rep[1] == 5 && table[1].rep[2] == -1 && table[1].rep[3] == -1);
  CHECK(table[1].vec == 0 && table[1].is_u8 && table[1].C == 10 && table[1].HW == 1);
  // an add block: its clip is the tail; without a clip it adds nothing
  tk_add_block_attrs ab{};
  ab.has_clip = 1, ab.clip_min = 7, ab.clip_max = 3;  // a_min wins
  const tk_tensor* outs3[2] = {&add.t, &clip.t};
  tk::ChainSpec sp3{TK_NODE_ADD_BLOCK, outs3, 2, nullptr, nullptr, nullptr, &ab};
  CHECK(tk::chain_append(sp3, "check", &table, &n_report, &blocks) == TK_OK);
  CHECK(table.size() == 3 && n_report == 7 && blocks == 5 && table[2].rep[3] == 6 && table[2].rep[0] == -1);
  CHECK(!table[2].has_i32 && table[2].clip_lo == 7 && table[2].clip_hi == 7 && (const void*)table[2].rq == add.t.data);
  ab.has_clip = 0;
  sp3.n_outs = 1;
  CHECK(tk::chain_append(sp3, "check", &table, &n_report, &blocks) == TK_OK && table.size() == 3 && n_report == 7);
  // records of no elements: entries, no workgroups
  Tensor e0(0, {0, 24, 9, 9}, TK_DL_INT, 32), e1(0, {0, 24, 9, 9}, TK_DL_INT, 32), e2(0, {0, 24, 9, 9}, TK_DL_INT, 8);
  const tk_tensor* outs4[3] = {&e0.t, &e1.t, &e2.t};
  tk_block_attrs at4{};
  Tensor bias4(0x30000, {24}, TK_DL_INT, 32);
  tk::ChainSpec sp4{TK_NODE_CONV_BLOCK, outs4, 3, &bias4.t, nullptr, &at4, nullptr};
  CHECK(tk::chain_append(sp4, "check", &table, &n_report, &blocks) == TK_OK && table.size() == 3 && n_report == 9 && blocks == 5);

  // refusals leave the table alone
  auto refused = [&](tk::ChainSpec s, const char* word) {
    const size_t before = table.size();
    tk::g_err.clear();
    const int rc = tk::chain_append(s, "check", &table, &n_report, &blocks);
    CHECK(rc == TK_ERR_INVALID_ARG && table.size() == before);
    CHECK(tk::g_err.find(word) != std::string::npos);
  };
  tk::ChainSpec bad = sp;
  bad.kind = TK_NODE_CLIP;
  refused(bad, "conv block");
  bad = sp, bad.outs = nullptr;
  refused(bad, "null");
  bad = sp, bad.bias = nullptr;
  refused(bad, "null");
  bad = sp, bad.residual = nullptr;
  refused(bad, "residual");
  bad = sp, bad.n_outs = 4;
  refused(bad, "outs");
  const tk_tensor* swapped[5] = {&rq.t, &bo.t, &rq.t, &add.t, &clip.t};
  bad = sp, bad.outs = swapped;
  refused(bad, "int32");
  Tensor clip_u8(0x15000, shape, TK_DL_UINT, 8);
  const tk_tensor* mixed[5] = {&conv.t, &bo.t, &rq.t, &add.t, &clip_u8.t};
  bad = sp, bad.outs = mixed;
  refused(bad, "dtype");
  Tensor strided = clip;
  strided.t.shape = strided.shape.data();
  int64_t st[4] = {1944, 81, 9, 1};
  strided.t.strides = st;
  const tk_tensor* with_strides[5] = {&conv.t, &bo.t, &rq.t, &add.t, &strided.t};
  bad = sp, bad.outs = with_strides;
  refused(bad, "compact");
  tk_block_attrs axis = at;
  axis.requantize.mode = TK_RQ_AXIS_UPWARD;
  bad = sp, bad.block = &axis;
  refused(bad, "multipliers");
  Tensor flat(0x1000, {5832}, TK_DL_INT, 32);
  const tk_tensor* one_d[1] = {&flat.t};
  bad = sp, bad.outs = one_d, bad.n_outs = 1;
  refused(bad, "channel axis");
  std::printf(g_fail ? "chain_table_check: %d failures\n" : "chain_table_check: ok\n", g_fail);
  return g_fail ? 1 : 0;
}
