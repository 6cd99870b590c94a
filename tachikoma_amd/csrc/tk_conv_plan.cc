// The conv / dense plan (tk_conv_plan.h).  Plain C++: every threshold below is a step of
// im2col_plan, evaluated once per plan, and its comment is the record of why it stands.
#include "tk_conv_plan.h"

#include <algorithm>

namespace tk {

// ---------------------------------------------------------------- geometry
int conv_geom(const tk_tensor* data, const tk_tensor* weight, const tk_conv2d_attrs* a, ConvGeom* g) {
  if (data->ndim != 4 || weight->ndim != 4) return TK_ERR_SHAPE;
  g->N = (int)data->shape[0];
  g->C = (int)data->shape[1];
  g->H = (int)data->shape[2];
  g->W = (int)data->shape[3];
  g->O = (int)weight->shape[0];
  g->KH = (int)weight->shape[2];
  g->KW = (int)weight->shape[3];
  int groups = a ? a->groups : 1;
  if (groups < 1 || g->C % groups || g->O % groups || weight->shape[1] * groups != g->C) return TK_ERR_SHAPE;
  if (a) {
    int dh = a->dilation[0], dw = a->dilation[1];
    g->OH = (g->H + a->padding[0] + a->padding[2] - dh * (g->KH - 1) - 1) / a->strides[0] + 1;
    g->OW = (g->W + a->padding[1] + a->padding[3] - dw * (g->KW - 1) - 1) / a->strides[1] + 1;
  }
  g->cin_pad = (g->C + 15) / 16 * 16;
  int k = g->KH * g->KW * g->cin_pad;
  g->k_pad = (k + kBK - 1) / kBK * kBK;
  g->k_eff = g->KH * g->KW * g->C;
  g->rows_pad = (g->O + 127) / 128 * 128;
  return TK_OK;
}

bool use_mfma_conv(const ConvGeom& g, int groups) { return groups == 1 && g.O >= 16 && g.C >= 3; }

// ---------------------------------------------------------------- traits
ConvTraits conv_traits(const ConvGeom& g, bool weight_u8, const tk_conv2d_attrs& a, bool block,
                       const tk_block_attrs* blk, bool shadow) {
  ConvTraits t{};
  t.block = block;
  t.zw = a.kernel_zero_point - (weight_u8 ? 128 : 0);
  t.zw_vec = a.kernel_zero_points != nullptr;
  t.patch = t.zw != 0 || t.zw_vec;
  t.has_add = blk && blk->has_add;
  t.in_pix = (int64_t)g.N * g.H * g.W;
  const int taps = g.KH * g.KW;
  t.unitap = taps <= 64 && (g.cin_pad % kBK == 0 || taps == 1) && env_int("TK_UNITAP", 1);
  {
    const int64_t hw = (int64_t)g.OH * g.OW;
    const uint64_t elems = (uint64_t)g.N * hw * g.O;
    // record stores are nontemporal (1) only where a plane's int32 rows are whole 128-byte
    // lines (or planes are tiny): measured on ResNet-50, partial-line NT stores (28x28, 14x14
    // planes) run up to 1.9x slower than plain ones, which the L2 merges before write-back
    const int epi = hw % 32 == 0 || hw <= 64 ? 1 : 2;
    t.fast_epi = blk && elems * 4 < 0xFFFFFFC0ull && hw % 4 == 0 && rq_fast_mode(blk->requantize.mode)
                     ? env_int("TK_FASTEPI", epi) : 0;
  }
  t.shadow = block && shadow;
  t.shadow_cpad = (g.O + 15) / 16 * 16;
  return t;
}

// ---------------------------------------------------------------- the im2col tile plan
namespace {

int ring_depth() {
  const char* e = tune_env("TK_RING");
  const int r = e ? atoi(e) : 3;
  return r >= 3 && r <= 5 ? r : 3;
}

// 64-row (MT = 1) tiles for conv blocks, except 128-channel layers with K >= 512, where one
// 128-row tile (MT = 2) per N tile measured 7-18% faster (ResNet-50's 28x28 stage: the B
// operand is staged once for both M halves); plain convs use MT = 2 above 64 channels.
// The 256-channel 3x3 layers of the 14x14 stage (K = 2304) also take 128-row tiles while the grid
// keeps >= 192 of them: half the im2col B re-reads per CU, -10 % (profiles/r02q_mt2_ab.txt).
bool conv_mt1(const ConvGeom& g, bool block) {
  if (g.O <= 64) return true;
  if (!block || tune_env("TK_MT2")) return false;
  if (g.O == 128 && g.k_eff >= 512 && env_int("TK_MT2_128", 1)) return false;
  const int64_t mt2_tiles = ((int64_t)g.N * g.OH * g.OW + 127) / 128 * ((g.O + 127) / 128);
  return !(g.O == 256 && g.k_eff >= 2048 && mt2_tiles >= 192 && env_int("TK_MT2_256", 1));
}

// 256-column tiles over the flattened pixel axis (BN = 256, no image alignment) for the short-K,
// >= 256-channel conv blocks on planes of more than 256 pixels (the 56x56 / 28x28 expand and
// downsample layers): each store instruction writes one 1 KB segment of a channel row instead of
// two 512-byte ones (store probe: -10 % on these layers' record writes,
// profiles/r02j_store_patterns.txt "span 64x256").  Off (TK_BN256_ROWS=1 in the ablation build):
// on the kernel the halved occupancy (2 workgroups per CU for 70 KB of LDS) costs more than the
// store pattern gains, the 56x56 expand with its residual join +19 % (profiles/r02s_bn256_rows_ab.txt).
bool conv_bn256_rows(const ConvGeom& g, bool block, bool patch) {
  const int64_t hw = (int64_t)g.OH * g.OW, P = (int64_t)g.N * hw;
  if (!block || patch || hw <= 256 || hw % 4 != 0 || g.O < 256 || g.k_pad > 256 ||
      P * g.O * 4 >= 0xFFFFFFC0ll || !env_int("TK_BN256_ROWS", 0))
    return false;
  return (P + 255) / 256 * ((g.O + 63) / 64) >= 256;
}

// 256-column image tiles (BN = 256) for conv blocks whose planes hold 65..256 pixels (14x14):
// floor(256 / HW) whole images per tile, so that each tile's records are contiguous runs
// (probe: 2x the store rate of 128-column tiles that cross images on 14x14 planes,
// profiles/r02j_store_patterns.txt).  Only where the grid still gives every CU a tile (no
// split-K), with the flat epilogue's preconditions.  Returns images per tile, or 0.
int conv_bn256_ipt(const ConvGeom& g, bool block, bool patch) {
  const int64_t hw = (int64_t)g.OH * g.OW;
  // short reductions only (the store-bound expand layers): a long K loop at the one or two
  // workgroups per CU of these tiles ran 15-20 % slower than 128-column tiles (3x3 256->256 and
  // 1x1 1024->256 at 14x14, profiles/r02n_bn256_ab.txt)
  if (!block || patch || hw <= 64 || hw > 256 || g.O % 4 != 0 || (int64_t)g.N * hw * g.O * 4 >= 0xFFFFFFC0ll ||
      g.k_pad > env_int("TK_BN256_KMAX", 256) || !env_int("TK_BN256", 1))
    return 0;
  const int ipt = (int)(256 / hw);
  const int64_t tiles = ((int64_t)g.N + ipt - 1) / ipt * ((g.O + 63) / 64);
  return tiles >= 256 ? ipt : 0;
}

// Images per N tile of a conv block whose planes hold 1..64 pixels (0: plain 128-column
// tiles).  Needs the flat epilogue's preconditions: no per-pixel zero-point patch, a channel
// count that keeps every image run 16-byte aligned, and 32-bit record offsets.
int conv_image_tiles(const ConvGeom& g, bool block, bool patch) {
  const int64_t hw = (int64_t)g.OH * g.OW;
  if (!block || patch || hw > 64 || g.O % 4 != 0 || (int64_t)g.N * hw * g.O * 4 >= 0xFFFFFFC0ll ||
      !env_int("TK_IMGTILE", 1))
    return 0;
  return (int)(128 / hw);
}

int64_t conv_ntiles(const ConvGeom& g, int ipt) {
  return ipt ? ((int64_t)g.N + ipt - 1) / ipt : ((int64_t)g.N * g.OH * g.OW + 127) / 128;
}

// Wide (128-byte) K stages: >= 8 steps of 64 bytes, every stage within one tap
// (cin_pad % 128 == 0).
bool wide_stages_fit(const ConvGeom& g) { return g.KH * g.KW <= 64 && g.cin_pad % 128 == 0 && g.k_pad / kBK >= 8; }

// ... for conv blocks on 64-row tiles with long reductions on small grids: few enough tiles that the
// 2 workgroups per CU the wide ring's LDS allows hold the whole grid (TK_WIDE_MAX_TILES).
bool conv_wide(const ConvGeom& g, bool block, int64_t tiles) {
  if (!block || !wide_stages_fit(g) || !env_int("TK_WIDE", 1) || !env_int("TK_UNITAP", 1) || tune_env("TK_MT2"))
    return false;
  // (256-column tiles, were it not for a patch: the wide ring holds one workgroup per CU)
  return tiles <= (conv_bn256_ipt(g, block, false) ? 256 : env_int("TK_WIDE_MAX_TILES", 512));
}

// ... and on 128-row tiles (96 KB ring, one workgroup per CU) where the grid fits one round: the
// 14x14 3x3 256-channel layers, -5.5 % (profiles/r02z_wide_mt2_ab.txt)
bool wide_mt2(const ConvGeom& g, bool block, int64_t tiles) {
  return block && wide_stages_fit(g) && tiles <= 256 && env_int("TK_WIDE_MT2", 1);
}

// Split-K of an MFMA conv: layers whose tile grid cannot give every CU a workgroup (the 7x7 stage
// at 64 samples) split the reduction so that ~3 workgroups per CU stay resident (each split keeps
// >= 6 k-steps); kper = k-steps per split.
void conv_split(int64_t tiles, int nk, bool mt1, int* splits, int* kper) {
  *splits = 1;
  *kper = nk;
  // measured: splitting grids of >= 256 tiles (one per CU) loses more to the partial-tile
  // round trip than it gains in latency hiding
  if (!mt1 || tiles >= 256) return;
  const int want = (int)std::min<int64_t>((768 + tiles - 1) / tiles, nk / 6);
  if (want <= 1) return;
  *kper = (nk + want - 1) / want;
  *splits = (nk + *kper - 1) / *kper;
}

// Split-K of a dense GEMM (MT = 2 tiles, 128 x 128): classifier heads have a handful of
// tiles and a long K (ResNet-50 fc: 8 tiles, 32 k-steps), so split until ~512 workgroups
// run, keeping >= 2 k-steps per split.
void dense_split(int64_t tiles, int nk, int* splits, int* kper) {
  *splits = 1;
  *kper = nk;
  if (tiles >= 256) return;
  // the reduce pass reads splits sequentially: a few splits already fill the chip
  const int want = (int)std::min<int64_t>(std::min<int64_t>((512 + tiles - 1) / tiles, nk / 2), 4);
  if (want <= 1) return;
  *kper = (nk + want - 1) / want;
  *splits = (nk + *kper - 1) / *kper;
}

// ints of one partial tile: 16 accumulators x 2 column tiles per 64 rows, for every thread
constexpr int64_t tile_ints(int mt) { return (int64_t)mt * 2 * 16 * kGemmThreads; }

}  // namespace

Im2colPlan im2col_plan(const ConvGeom& g, const ConvTraits& t) {
  const int64_t hw = (int64_t)g.OH * g.OW, P = (int64_t)g.N * hw;
  Im2colPlan p{};
  const bool mt1 = conv_mt1(g, t.block);
  p.mt = mt1 ? 1 : 2;
  // N tiles: whole images (256 columns, else 128), 256 flat columns, or 128 flat columns
  const int ipt256 = mt1 ? conv_bn256_ipt(g, t.block, t.patch) : 0;
  p.ipt = ipt256 ? ipt256 : mt1 ? conv_image_tiles(g, t.block, t.patch) : 0;
  const bool rows256 = mt1 && !p.ipt && conv_bn256_rows(g, t.block, t.patch);
  p.bn = ipt256 || rows256 ? 256 : 128;
  p.tcols = p.ipt ? p.ipt * (int)hw : p.bn;
  p.ntiles = rows256 ? (int32_t)((P + 255) / 256) : (int32_t)conv_ntiles(g, p.ipt);
  p.ntiles8 = (p.ntiles + 7) / 8 * 8;
  p.mtiles = (g.O + 64 * p.mt - 1) / (64 * p.mt);
  // (the tile count the wide and split steps were measured against takes 128 flat columns where
  // the tiles hold no whole images)
  const int64_t tiles = conv_ntiles(g, p.ipt) * p.mtiles;
  p.wide = mt1 ? conv_wide(g, t.block, tiles) : wide_mt2(g, t.block, (int64_t)p.mtiles * p.ntiles);
  conv_split(tiles, g.k_pad / (p.wide && mt1 ? 2 * kBK : kBK), mt1, &p.splits, &p.kper);
  p.partial_bytes = p.splits > 1 ? tiles * p.splits * tile_ints(p.mt) * 4 : 0;
  // the ring depth is an A/B knob of the 64-row kernels on 128-column tiles (a split's wide partial
  // pass has the one depth)
  const bool split = p.splits > 1;
  p.ring = mt1 && p.bn == 128 && (split ? !p.wide : t.block) ? ring_depth() : 3;
  p.main = split ? GemmVariant{1, true, false, 1, p.ring, p.wide, 128}
                 : GemmVariant{p.mt, true, t.block, 0, p.ring, p.wide, p.bn};
  p.reduce = GemmVariant{1, true, t.block, 2, 3, false, 128};
  return p;
}

// ---------------------------------------------------------------- layouts
ConvScratch conv_scratch(const ConvGeom& g, const ConvTraits& t, const Im2colPlan& p, int64_t other_bytes) {
  ConvScratch s{};
  s.patch = 0;
  s.partials = t.patch ? al256((int64_t)g.N * g.OH * g.OW * 4) : 0;
  s.bytes = s.partials + std::max(al256(p.partial_bytes), al256(other_bytes));
  return s;
}

ConvWorkspace conv_workspace(const ConvGeom& g, int64_t packed_bytes, int64_t shadow_bytes, int64_t scratch_bytes) {
  ConvWorkspace w{};
  w.packed = 0;
  w.sums = w.packed + al256(packed_bytes);
  w.shadow = w.sums + al256((int64_t)g.rows_pad * 4);
  w.scratch = w.shadow + al256(shadow_bytes);
  w.bytes = w.scratch + scratch_bytes;
  return w;
}

DensePlan dense_plan(int64_t M, int64_t N, int64_t K, bool block) {
  DensePlan d{};
  d.k_pad = (int)((K + kBK - 1) / kBK * kBK);
  d.mrows = (int)((M + 127) / 128 * 128);
  d.nrows = (int)((N + 127) / 128 * 128);
  d.ntiles = (int32_t)((N + 127) / 128);
  d.ntiles8 = (d.ntiles + 7) / 8 * 8;
  d.mtiles = (int32_t)((M + 127) / 128);
  const int64_t tiles = (int64_t)d.mtiles * d.ntiles;
  dense_split(tiles, d.k_pad / kBK, &d.splits, &d.kper);
  d.pad_a = 0;
  d.pad_b = d.pad_a + al256((int64_t)d.mrows * d.k_pad);
  d.sum_a = d.pad_b + al256((int64_t)d.nrows * d.k_pad);
  d.sum_b = d.sum_a + al256((int64_t)d.mrows * 4);
  d.partials = d.sum_b + al256((int64_t)d.nrows * 4);
  d.bytes = d.partials + al256(d.splits > 1 ? tiles * d.splits * tile_ints(2) * 4 : 0);
  d.main = d.splits > 1 ? GemmVariant{2, false, false, 1, 3, false, 128} : GemmVariant{2, false, block, 0, 3, false, 128};
  d.reduce = GemmVariant{2, false, block, 2, 3, false, 128};
  return d;
}

}  // namespace tk
