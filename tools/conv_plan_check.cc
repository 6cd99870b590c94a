// Stand-alone check of the conv / dense plan (csrc/tk_conv_plan.cc) for sanitizer builds: sweeps
// batch, plane, channel, kernel and stride sizes with the block and the patch on and off, and checks
// every plan against what the kernels and the scratch carving assume of it.  It inspects the
// project's own plan, no compiled code.  CPU only; never needs a device.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/conv_plan_check.cc tachikoma_amd/csrc/tk_conv_plan.cc -o conv_plan_check && ./conv_plan_check
//
// The ring 4 and 5 keys exist only in the ablation build, whose plans follow TK_RING: the same line
// with -DTK_ABLATION_BUILD -o conv_plan_check_abl, then
//   TK_RING=4 ./conv_plan_check_abl && TK_RING=5 ./conv_plan_check_abl
// sweeps them (a split's wide partial pass, 256-column and 128-row tiles must stay at ring 3).
#include <cstdint>
#include <cstdio>
#include <string>

#include "../tachikoma_amd/csrc/tk_conv_plan.h"

namespace tk {
void set_error(const std::string&) {}
}  // namespace tk

static long g_fail = 0, g_plans = 0;
static long g_seen[6];  // plans with 128-row tiles, 256 columns, image tiles, wide stages, a split, a patch
static long g_other_ring;  // plans at ring 4 or 5 (ablation build under TK_RING)
static std::string g_case;
#define CHECK(c)                                                                      \
  do {                                                                                \
    if (!(c)) {                                                                       \
      if (g_fail < 20) std::printf("FAIL %s:%d %s  [%s]\n", __FILE__, __LINE__, #c, g_case.c_str()); \
      ++g_fail;                                                                       \
    }                                                                                 \
  } while (0)

static void check_conv(int N, int C, int H, int W, int O, int KH, int KW, int stride, bool block, bool patch) {
  int64_t xs[4] = {N, C, H, W}, ws[4] = {O, C, KH, KW};
  tk_tensor x{}, w{};
  x.ndim = w.ndim = 4;
  x.shape = xs;
  w.shape = ws;
  x.dtype = w.dtype = {TK_DL_INT, 8, 1};
  tk_conv2d_attrs a{};
  a.strides[0] = a.strides[1] = stride;
  a.padding[0] = a.padding[2] = KH / 2;
  a.padding[1] = a.padding[3] = KW / 2;
  a.dilation[0] = a.dilation[1] = 1;
  a.groups = 1;
  a.kernel_zero_point = patch ? 2 : 0;
  tk::ConvGeom g;
  if (tk::conv_geom(&x, &w, &a, &g) != TK_OK || g.OH < 1 || g.OW < 1 || !tk::use_mfma_conv(g, 1)) return;
  g_case = std::to_string(N) + "x" + std::to_string(C) + "x" + std::to_string(H) + "x" + std::to_string(W) + " -> " +
           std::to_string(O) + " k" + std::to_string(KH) + "x" + std::to_string(KW) + " s" + std::to_string(stride) +
           (block ? " block" : "") + (patch ? " patch" : "");
  tk_block_attrs blk{};
  blk.conv = a;
  blk.requantize.mode = TK_RQ_AXIS_UPWARD;
  const tk::ConvTraits t = tk::conv_traits(g, false, a, block, block ? &blk : nullptr, block);
  CHECK(t.block == block && t.patch == patch);
  const tk::Im2colPlan p = tk::im2col_plan(g, t);
  ++g_plans;
  g_seen[0] += p.mt == 2, g_seen[1] += p.bn == 256, g_seen[2] += p.ipt > 0, g_seen[3] += p.wide, g_seen[4] += p.splits > 1,
      g_seen[5] += t.patch;
  const int64_t hw = (int64_t)g.OH * g.OW, P = (int64_t)g.N * hw;
  // variant: the kernels the plan names exist
  CHECK(tk::gemm_variant_exists(p.main));
  if (p.splits > 1) CHECK(tk::gemm_variant_exists(p.reduce));
  CHECK(p.main.im2col && p.main.mt == (p.splits > 1 ? 1 : p.mt) && p.main.wide == p.wide && p.main.ring == p.ring);
  CHECK(p.main.mode == (p.splits > 1 ? 1 : 0) && p.main.block == (p.splits > 1 ? false : block));
  CHECK(p.reduce.mode == 2 && p.reduce.block == block);
  // tile count: the grid is padded to whole rounds of the 8 XCDs, and the tiles cover every pixel and row
  CHECK((p.mt == 1 || p.mt == 2) && (p.bn == 128 || p.bn == 256));
  CHECK(p.ntiles8 % 8 == 0 && p.ntiles8 >= p.ntiles && p.ntiles >= 1);
  CHECK((int64_t)p.mtiles * 64 * p.mt >= g.O && (int64_t)(p.mtiles - 1) * 64 * p.mt < g.O);
  // tile columns
  CHECK(p.tcols >= 1 && p.tcols <= p.bn);
  if (p.ipt) {
    CHECK((int64_t)p.ipt * hw == p.tcols);
    CHECK((int64_t)p.ntiles * p.ipt >= g.N && (int64_t)(p.ntiles - 1) * p.ipt < g.N);
  } else {
    CHECK(p.tcols == p.bn);
    CHECK((int64_t)p.ntiles * p.tcols >= P && (int64_t)(p.ntiles - 1) * p.tcols < P);
  }
  // split: no empty split
  const int nk = g.k_pad / (p.wide && p.mt == 1 ? 2 * tk::kBK : tk::kBK);
  CHECK(p.splits >= 1 && p.kper >= 1);
  CHECK((int64_t)p.splits * p.kper >= nk && nk > (int64_t)(p.splits - 1) * p.kper);
  if (p.splits > 1) CHECK(p.mt == 1);
  // partial size: register-order tiles of MT * 2 * 16 ints per thread
  const int64_t tile_ints = (int64_t)p.mt * 2 * 16 * tk::kGemmThreads;
  CHECK(p.partial_bytes == (p.splits > 1 ? (int64_t)p.mtiles * p.ntiles * p.splits * tile_ints * 4 : 0));
  // 256-column tiles
  if (p.bn == 256) CHECK(p.mt == 1 && p.splits == 1 && block);
  // wide stages: every 128-byte stage within one tap
  if (p.wide) CHECK(g.cin_pad % 128 == 0 && g.k_pad % 128 == 0 && block);
  if (p.ring != 3) CHECK(p.mt == 1 && p.bn == 128 && !(p.splits > 1 && p.wide) && (p.splits > 1 || block));
  g_other_ring += p.ring != 3;
  // scratch: covers the patch sums plus the partials, which do not overlap
  for (int64_t other : {(int64_t)0, (int64_t)1000}) {
    const tk::ConvScratch s = tk::conv_scratch(g, t, p, other);
    CHECK(s.patch == 0 && s.partials % 256 == 0 && s.partials >= (patch ? P * 4 : 0));
    CHECK(s.bytes >= s.partials + p.partial_bytes && s.bytes >= s.partials + other);
    if (!patch && p.splits == 1 && !other) CHECK(s.bytes == 0);
  }
  const tk::ConvWorkspace wk = tk::conv_workspace(g, 1000, 777, 512);
  CHECK(wk.packed == 0 && wk.sums >= 1000 && wk.shadow >= wk.sums + (int64_t)g.rows_pad * 4 &&
        wk.scratch >= wk.shadow + 777 && wk.bytes == wk.scratch + 512);
  CHECK(wk.sums % 256 == 0 && wk.shadow % 256 == 0 && wk.scratch % 256 == 0);
}

static void check_dense(int64_t M, int64_t N, int64_t K, bool block) {
  g_case = "dense " + std::to_string(M) + "x" + std::to_string(K) + " x " + std::to_string(N);
  const tk::DensePlan d = tk::dense_plan(M, N, K, block);
  ++g_plans;
  CHECK(tk::gemm_variant_exists(d.main));
  if (d.splits > 1) CHECK(tk::gemm_variant_exists(d.reduce));
  CHECK(d.k_pad % tk::kBK == 0 && d.k_pad >= K && d.mrows % 128 == 0 && d.mrows >= M && d.nrows % 128 == 0 && d.nrows >= N);
  CHECK(d.ntiles8 % 8 == 0 && d.ntiles8 >= d.ntiles && d.ntiles * 128 == d.nrows && d.mtiles * 128 == d.mrows);
  const int nk = d.k_pad / tk::kBK;
  CHECK((int64_t)d.splits * d.kper >= nk && nk > (int64_t)(d.splits - 1) * d.kper);
  // the regions do not overlap and sum to the reported size
  const int64_t partial = d.splits > 1 ? (int64_t)d.mtiles * d.ntiles * d.splits * (2 * 2 * 16 * tk::kGemmThreads) * 4 : 0;
  const int64_t off[6] = {d.pad_a, d.pad_b, d.sum_a, d.sum_b, d.partials, d.bytes};
  const int64_t len[5] = {(int64_t)d.mrows * d.k_pad, (int64_t)d.nrows * d.k_pad, (int64_t)d.mrows * 4,
                          (int64_t)d.nrows * 4, partial};
  CHECK(off[0] == 0);
  for (int i = 0; i < 5; ++i) CHECK(off[i] % 256 == 0 && off[i + 1] == tk::al256(off[i] + len[i]));
}

int main() {
  const int sizes[] = {3, 16, 24, 64, 96, 128, 256, 512, 1000, 2048};
  const int kernels[][2] = {{1, 1}, {3, 3}, {7, 7}, {1, 7}};
  for (int N : {1, 2, 3, 16, 64, 65})
    for (int H = 1; H <= 57; ++H)
      for (int W : {H, H == 1 ? 5 : (H + 1) / 2, 57})  // square and two non-square planes
        for (int C : sizes)
          for (int O : sizes)
            for (const auto& k : kernels)
              for (int stride : {1, 2})
                for (int flags = 0; flags < 4; ++flags) check_conv(N, C, H, W, O, k[0], k[1], stride, flags & 1, flags & 2);
  for (int64_t M : {1, 5, 64, 130, 1000})
    for (int64_t N : {1, 10, 129, 1000, 4096})
      for (int64_t K : {1, 70, 84, 512, 2048, 25088})
        for (bool block : {false, true}) check_dense(M, N, K, block);
  g_case = "sweep";
#ifdef TK_ABLATION_BUILD
  if (const char* r = getenv("TK_RING")) CHECK((atoi(r) == 4 || atoi(r) == 5) == (g_other_ring > 0));
#else
  CHECK(g_other_ring == 0);
#endif
  for (long n : g_seen) CHECK(n > 0);  // the sweep reaches every kind of plan
  std::printf("conv_plan_check: %ld plans (%ld with 128-row tiles, %ld 256 columns, %ld image tiles, %ld wide stages, "
              "%ld split, %ld patch), %ld failures\n", g_plans, g_seen[0], g_seen[1], g_seen[2], g_seen[3], g_seen[4],
              g_seen[5], g_fail);
  return g_fail ? 1 : 0;
}
