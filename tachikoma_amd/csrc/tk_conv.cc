// qnn.conv2d and the fused conv block on the host: validate, plan (tk_conv_plan.h), launch.
//   conv2d_run     builds the geometry, the traits and -- for the im2col kernel -- the tile plan
//                  once, then hands the launch to the kernel the block's algo names: the dense tile
//                  kernel (tk_dense.hip), an image-tile plan (tk_conv_img.hip), the persistent kernel
//                  (tk_conv_pf.hip), else gemm_i8_kernel (tk_gemm.hip) by the plan's variant key;
//                  grouped / depthwise / tiny convs go to tk_dw.hip and tk_conv_direct.hip
//   the algo listing and the scratch / workspace sizes read the same traits and plan
#include <algorithm>
#include <climits>
#include <cstdio>
#include <string>

#include "tk_conv.h"
#include "tk_ops.h"

namespace tk {

// The plan's fast_epi rule (rq_fast_mode, plain C++) and the kernels' (block_rq_fast_mode,
// tk_block_tail.h) are one rule: fast_epi must never launch block_rq<true> for a mode the
// kernels reject, or the reverse.
static_assert(rq_fast_mode(TK_RQ_IDENTITY) == block_rq_fast_mode(TK_RQ_IDENTITY) &&
                  rq_fast_mode(TK_RQ_TENSOR_POW2) == block_rq_fast_mode(TK_RQ_TENSOR_POW2) &&
                  rq_fast_mode(TK_RQ_TENSOR_UPWARD) == block_rq_fast_mode(TK_RQ_TENSOR_UPWARD) &&
                  rq_fast_mode(TK_RQ_TENSOR_TONEAREST) == block_rq_fast_mode(TK_RQ_TENSOR_TONEAREST) &&
                  rq_fast_mode(TK_RQ_AXIS_UPWARD) == block_rq_fast_mode(TK_RQ_AXIS_UPWARD) &&
                  rq_fast_mode(TK_RQ_AXIS_TONEAREST) == block_rq_fast_mode(TK_RQ_AXIS_TONEAREST),
              "rq_fast_mode (tk_conv_plan.h) and block_rq_fast_mode (tk_block_tail.h) disagree");

static inline uint32_t rep4(int v) {
  uint32_t b = (uint8_t)(int8_t)v;
  return b | (b << 8) | (b << 16) | (b << 24);
}


// Validates a fused block and fills the epilogue part of GemmArgs.
int setup_block(GemmArgs& ga, const BlockIO* b, const tk_tensor* conv_out, int channels, int ch_axis) {
  if (!b) return TK_OK;
  const tk_block_attrs* at = b->attrs;
  TK_CHECK_ARG(at && b->outs && b->bias, "block needs bias, attrs and outputs");
  const int has_add = at->has_add ? 1 : 0;
  TK_CHECK_ARG(b->n_outs == 3 + has_add + (at->has_clip ? 1 : 0), "outs = {conv, bias_add, requantize, [add], [clip]}");
  TK_CHECK_ARG(is_int(b->bias, 32) && numel(b->bias) == channels, "bias must be int32 [channels]");
  const tk_tensor* bo = b->outs[1];
  const tk_tensor* rq = b->outs[2];
  TK_CHECK_ARG(is_int(bo, 32) && numel(bo) == numel(conv_out), "bias_add output must be int32, conv shaped");
  TK_CHECK_ARG(is_int8ish(rq) && numel(rq) == numel(conv_out), "requantize output must be int8/uint8, conv shaped");
  int rq_axis = at->requantize.axis;
  TK_CHECK_ARG(rq_axis == ch_axis || at->requantize.mode <= TK_RQ_TENSOR_TONEAREST,
               "requantize must run along the channel axis to fuse");
  for (int k = 3; k < b->n_outs; ++k)
    TK_CHECK_ARG(b->outs[k]->dtype.code == rq->dtype.code && b->outs[k]->dtype.bits == 8 &&
                     numel(b->outs[k]) == numel(conv_out) && compact(b->outs[k]),
                 "add / clip outputs must match the requantize output");
  if (has_add) {
    const tk_tensor* res = at->residual;
    TK_CHECK_ARG(res && dt_of(res) == dt_of(rq) && numel(res) == numel(conv_out) && compact(res),
                 "residual must match the requantize output (same shape and dtype)");
    TK_CHECK_ARG(at->add.lhs.mode <= TK_RQ_TENSOR_TONEAREST && at->add.rhs.mode <= TK_RQ_TENSOR_TONEAREST,
                 "qnn.add: per-tensor parameters only");
    const tk_requantize_attrs& blk_side = at->block_is_rhs ? at->add.rhs : at->add.lhs;
    const tk_requantize_attrs& res_side = at->block_is_rhs ? at->add.lhs : at->add.rhs;
    auto rqp = [](const tk_requantize_attrs& r) {
      RqParams q{};
      q.mode = r.mode;
      q.multiplier = r.multiplier;
      q.shift = r.shift;
      q.zp_in = r.input_zero_point;
      q.zp_out = r.output_zero_point;
      q.inner = 1;
      q.C = 1;
      return q;
    };
    ga.has_add = 1;
    ga.add_res = (const uint8_t*)ptr(res);
    ga.add_out = (uint8_t*)ptr(b->outs[3]);
    ga.add_pb = rqp(blk_side);
    ga.add_pr = rqp(res_side);
    ga.add_up_b = at->block_is_rhs ? at->add.rhs_upcast : at->add.lhs_upcast;
    ga.add_up_r = at->block_is_rhs ? at->add.lhs_upcast : at->add.rhs_upcast;
    ga.add_zp = at->add.output_zero_point;
  }
  ga.bias = (const int32_t*)ptr(b->bias);
  ga.bias_out = (int32_t*)ptr(bo);
  ga.rq_out = (uint8_t*)ptr(rq);
  ga.clip_out = at->has_clip ? (uint8_t*)ptr(b->outs[3 + has_add]) : nullptr;
  ga.has_clip = at->has_clip;
  bool u8 = is_uint(rq, 8);
  int64_t lo = u8 ? 0 : -128, hi = u8 ? 255 : 127;
  ga.clip_lo = (int32_t)std::max(at->clip_min, lo);
  // clip is max(min(x, a_max), a_min) (topi/math.py:634-638): a_min wins when a_min > a_max, which
  // the kernels' min(max(x, lo), hi) reproduces with hi raised to lo (and clamp_i32 needs lo <= hi)
  ga.clip_hi = (int32_t)std::max<int64_t>(std::min(at->clip_max, hi), ga.clip_lo);
  RqParams& p = ga.rq;
  p.mode = at->requantize.mode;
  p.multiplier = at->requantize.multiplier;
  p.shift = at->requantize.shift;
  p.zp_in = at->requantize.input_zero_point;
  p.zp_out = at->requantize.output_zero_point;
  p.ms = at->requantize.multipliers;
  p.ss = at->requantize.shifts;
  p.zps = at->requantize.input_zero_points;
  p.inner = 1;
  p.C = channels;
  p.qmin = lo;
  p.qmax = hi;
  p.clip_out = 1;
  if ((p.mode == TK_RQ_AXIS_UPWARD || p.mode == TK_RQ_AXIS_TONEAREST) && (!p.ms || !p.ss)) {
    set_error("block: per-axis requantize needs device multipliers/shifts");
    return TK_ERR_INVALID_ARG;
  }
  ga.shadow_out = (uint8_t*)b->shadow_out;
  ga.shadow_cpad = (channels + 15) / 16 * 16;
  ga.shadow_xor = u8 ? 0x80u : 0u;
  return TK_OK;
}

// Tile order (tile_of): on planes of up to 28x28 outputs, each XCD takes a contiguous run of N
// tiles, so the int32 record lines two neighbouring tiles share (rows of 784 B or less) are
// completed in one L2; on larger planes N tiles are striped over the XCDs (the 56x56 stage
// measured 5-7 % faster striped, the 28/14/7 stages 5-11 % faster chunked,
// profiles/r01e_ab_xcd_order.txt).  TK_XCD overrides (0 = plain order).
static int xcd_order(int64_t out_hw) {
  const char* e = tune_env("TK_XCD");
  return e ? atoi(e) : (out_hw <= 784 ? 2 : 1);
}

static int nt_stores() {
  const char* e = tune_env("TK_NT");
  return e ? atoi(e) : 1;
}

static int ablate_flags() {
  const char* e = tune_env("TK_ABLATE");
  return e ? atoi(e) : 0;
}

// scratch that the block kernels other than im2col need in place of its split's partial tiles
static int64_t other_scratch_bytes(const ConvGeom& g, const ConvTraits& t) {
  if (!t.block || t.patch) return 0;
  // the split-K image-tile plans' partial records, the dense head's K-slice sums
  return std::max(conv_img_split_scratch_bytes(g), conv_dense_scratch_bytes(g));
}

int64_t conv_scratch_bytes(const tk_tensor* data, const tk_tensor* weight, const tk_conv2d_attrs* a, int block) {
  if (!a) return -1;
  ConvGeom g;
  if (conv_geom(data, weight, a, &g) != TK_OK) return -1;
  if (!use_mfma_conv(g, a->groups)) return 0;
  const ConvTraits t = conv_traits(g, is_uint(weight, 8), *a, block != 0, nullptr, false);
  return conv_scratch(g, t, im2col_plan(g, t), other_scratch_bytes(g, t)).bytes;
}

// The operands and the im2col geometry of an MFMA conv's GemmArgs.
static void conv_gemm_args(GemmArgs& ga, const ConvGeom& g, const tk_conv2d_attrs* a, const ConvTraits& t, int32_t za,
                           const void* shadow, const void* packed, const int32_t* sums) {
  const int64_t P = (int64_t)g.N * g.OH * g.OW;
  ga.A = (const int8_t*)packed;
  ga.B = (const int8_t*)shadow;
  ga.lda = g.k_pad;
  ga.ldb = g.cin_pad;
  ga.k_pad = g.k_pad;
  ga.k_eff = g.k_eff;
  // operand A = weights (zero point zw), operand B = activations (zero point za)
  ga.zA = t.zw;
  ga.zB = za;
  ga.RA = sums;
  ga.H = g.H; ga.W = g.W; ga.cin_pad = g.cin_pad; ga.KH = g.KH; ga.KW = g.KW;
  ga.in_pix = t.in_pix;
  ga.sh = a->strides[0]; ga.sw = a->strides[1]; ga.pt = a->padding[0]; ga.pl = a->padding[1];
  ga.dh = a->dilation[0]; ga.dw = a->dilation[1];
  ga.taps = g.KH * g.KW;
  ga.cgroups = g.cin_pad / 16;
  ga.unitap = t.unitap;
  {
    // (p * ceil(2^40 / d)) >> 40 == p / d while p * d < 2^40
    const uint64_t hw = (uint64_t)g.OH * g.OW;
    auto magic = [](uint64_t d, uint64_t pmax) -> uint64_t {
      return pmax * d < (1ull << 40) ? ((1ull << 40) + d - 1) / d : 0;
    };
    ga.mg_hw = magic(hw, (uint64_t)P);
    ga.mg_ow = magic((uint64_t)g.OW, hw);
  }
  ga.fill = rep4(za);
  ga.out_elems = (uint32_t)std::min<uint64_t>((uint64_t)P * g.O, 0xFFFFFFFFull);
  ga.fast_epi = t.fast_epi;
  ga.out_nchw = 1;
  ga.vecw = g.OH * g.OW % 4 == 0 ? 4 : 1;  // store vectors must not straddle an image plane
}

static int conv2d_run(const tk_tensor* data, const void* shadow, const tk_tensor* weight, const void* packed,
                      const int32_t* sums, tk_tensor* out, const tk_conv2d_attrs* a, void* scratch,
                      const BlockIO* blk, hipStream_t s) {
  TK_CHECK_ARG(data && weight && out && a, "null argument");
  TK_CHECK_ARG(is_int8ish(data) && is_int8ish(weight) && is_int(out, 32), "dtypes: int8/uint8 in, int32 out");
  ConvGeom g;
  if (conv_geom(data, weight, a, &g) != TK_OK) {
    set_error("tk_qnn_conv2d: bad shapes");
    return TK_ERR_SHAPE;
  }
  TK_CHECK_ARG(out->ndim == 4 && out->shape[0] == g.N && out->shape[1] == g.O && out->shape[2] == g.OH &&
                   out->shape[3] == g.OW,
               "output shape mismatch");
  TK_CHECK_ARG(a->strides[0] > 0 && a->strides[1] > 0 && a->dilation[0] > 0 && a->dilation[1] > 0, "bad strides");
  int64_t P = (int64_t)g.N * g.OH * g.OW;
  TK_CHECK_ARG(P < INT32_MAX && (int64_t)g.N * g.O * g.OH * g.OW < INT32_MAX * 2LL, "tensor too large");
  GemmArgs ga{};
  ga.C = (int32_t*)ptr(out);
  ga.M = g.O;
  ga.N = (int32_t)P;
  ga.OH = g.OH;
  ga.OW = g.OW;
  ga.ch_is_row = 1;
  ga.ablate = ablate_flags();
  ga.nt = nt_stores();
  ga.xcd_order = xcd_order((int64_t)g.OH * g.OW);
  int rc = setup_block(ga, blk, out, g.O, 1);
  if (rc) return rc;
  if (!use_mfma_conv(g, a->groups)) {
    TK_CHECK_ARG(!(blk && blk->attrs->has_add), "residual join needs an MFMA conv block");
    // depthwise 3x3 blocks, every plane size: the tile kernel of tk_dw.hip (TK_DW2=0 in the
    // ablation build keeps the older band / direct kernels for A/B)
    if (blk && env_int("TK_DW2", 1)) {
      int rc_dw = TK_OK;
      if (dw_block_try(data, weight, g, a, ga, s, &rc_dw)) return rc_dw;
    }
    return conv_direct_run(data, weight, g, a, ga, blk != nullptr, s);
  }
  TK_CHECK_ARG(shadow && packed && sums, "MFMA conv needs shadow, packed weight and weight sums");
  const bool wu = is_uint(weight, 8);
  TK_CHECK_ARG(!(wu && a->kernel_zero_points), "per-channel zero points with uint8 weights are not supported");
  const tk_block_attrs* at = blk ? blk->attrs : nullptr;
  const ConvTraits t = conv_traits(g, wu, *a, blk != nullptr, at, blk && blk->shadow_out);
  conv_gemm_args(ga, g, a, t, a->input_zero_point - (is_uint(data, 8) ? 128 : 0), shadow, packed, sums);
  const Im2colPlan p = im2col_plan(g, t);
  const ConvScratch lay = conv_scratch(g, t, p, 0);
  if (t.patch) {
    TK_CHECK_ARG(scratch, "non-zero kernel zero point needs scratch (tk_conv2d_scratch_bytes)");
    int32_t* ps = (int32_t*)((char*)scratch + lay.patch);
    rc = conv_patch_sums(shadow, ps, ga, g.C, s);
    if (rc) return rc;
    ga.RB = ps;
    ga.zA_vec = a->kernel_zero_points;
  }
  char* sc = (char*)scratch + lay.partials;  // what follows the patch sums
  const int algo = at ? at->algo : 0;
  if (algo == kAlgoDense) {
    if (!conv_dense_applies(g, t)) {
      set_error("tk_qnn_conv2d_block: algo 5 (dense tiles) does not apply to this block; see tk_conv2d_block_algos");
      return TK_ERR_INVALID_ARG;
    }
    return conv_dense_run(g, t, ga, sc, s);
  }
  if (blk) {
    // whole-image tiles with the patch staged per channel stage (tk_conv_img.hip) where they apply
    const int8_t* chunked = conv_img_chunked_bytes(g.rows_pad, g.cin_pad, g.KH * g.KW)
                                ? (const int8_t*)packed + (int64_t)g.rows_pad * g.k_pad
                                : nullptr;
    int irc = TK_OK;
    if (conv_img_try(g, a, t, ga, chunked, sc, algo, s, &irc)) return irc;
    if (algo == kAlgoPf2 || algo == kAlgoPf3) {
      if (!conv_pf_applies(g, t)) {
        set_error("tk_qnn_conv2d_block: algo " + std::to_string(algo) +
                  " (persistent im2col) does not apply to this conv; see tk_conv2d_block_algos");
        return TK_ERR_INVALID_ARG;
      }
      return conv_pf_run(g, ga, algo == kAlgoPf2 ? 2 : 3, s);
    }
  }
  ga.ipt = p.ipt;
  ga.tcols = p.tcols;
  ga.ntiles = p.ntiles;
  ga.ntiles8 = p.ntiles8;
  ga.mtiles = p.mtiles;
  const dim3 grid((unsigned)((int64_t)p.mtiles * p.ntiles8));
  if (p.splits > 1) {
    TK_CHECK_ARG(scratch, "split-K conv needs scratch (tk_conv2d_scratch_bytes)");
    ga.ws = (int32_t*)sc;
    ga.splits = p.splits;
    ga.kper = p.kper;
    rc = gemm_launch(p.main, dim3(grid.x, 1, (unsigned)p.splits), 0, ga, s);
    return rc ? rc : gemm_launch(p.reduce, grid, 0, ga, s);
  }
  // profiling: extra LDS per workgroup of the 64-row block kernel
  const unsigned pad = p.mt == 1 && p.bn == 128 && t.block ? (unsigned)env_int("TK_LDS_PAD", 0) : 0;
  return gemm_launch(p.main, grid, pad, ga, s);
}

int conv2d_prepared_impl(const tk_tensor* data, const void* shadow, const tk_tensor* weight, const void* packed,
                         const int32_t* sums, tk_tensor* out, const tk_conv2d_attrs* a, void* workspace_patch,
                         hipStream_t s) {
  return conv2d_run(data, shadow, weight, packed, sums, out, a, workspace_patch, nullptr, s);
}

int conv2d_block_impl(const tk_tensor* data, const void* shadow, const tk_tensor* weight, const void* packed,
                      const int32_t* sums, const tk_tensor* bias, tk_tensor* const* outs, int n_outs,
                      const tk_block_attrs* attrs, void* patch, void* shadow_out, hipStream_t s) {
  TK_CHECK_ARG(outs && n_outs >= 3 && outs[0], "block needs outputs");
  BlockIO b{bias, outs, n_outs, attrs, shadow_out};
  return conv2d_run(data, shadow, weight, packed, sums, outs[0], attrs ? &attrs->conv : nullptr, patch, &b, s);
}

// The traits of a block as the listing sees it: conv2d_run's, for a block that writes its shadow
// (the shadow is bounded like the records, so that every algo listed here runs there either way).
static ConvTraits listing_traits(const ConvGeom& g, const tk_tensor* weight, const tk_block_attrs* attrs) {
  return conv_traits(g, is_uint(weight, 8), attrs->conv, true, attrs, true);
}

static bool have_chunked(const ConvGeom& g) {
  return g.KH * g.KW == 1 || conv_img_chunked_bytes(g.rows_pad, g.cin_pad, g.KH * g.KW);
}

int conv2d_block_algo_info_impl(const tk_tensor* data, const tk_tensor* weight, const tk_block_attrs* attrs, int algo,
                                char* buf, int len) {
  TK_CHECK_ARG(data && weight && attrs && buf && len > 0, "null argument");
  ConvGeom g;
  if (conv_geom(data, weight, &attrs->conv, &g) != TK_OK) {
    set_error("tk_conv2d_block_algo_info: bad shapes");
    return TK_ERR_SHAPE;
  }
  const char* fixed = algo == kAlgoIm2col ? "im2col tiles (64 or 128 rows x 128 or 256 columns, the library's own shape)"
                      : algo == kAlgoPf2  ? "persistent im2col tiles, 2 workgroups per CU"
                      : algo == kAlgoPf3  ? "persistent im2col tiles, 1 workgroup per CU (3-slot ring)"
                      : algo == kAlgoDense ? "dense tiles: 32 units x 64 samples, K split over 8 waves"
                                           : nullptr;
  if (fixed) {
    std::snprintf(buf, (size_t)len, "%s", fixed);
    return TK_OK;
  }
  const int rc = conv_img_describe(g, &attrs->conv, listing_traits(g, weight, attrs), have_chunked(g), algo, buf, len);
  if (rc) set_error("tk_conv2d_block_algo_info: algo " + std::to_string(algo) + " is not listed for this block");
  return rc;
}

int conv2d_block_algos_impl(const tk_tensor* data, const tk_tensor* weight, const tk_block_attrs* attrs,
                            int32_t* algos, int max_algos) {
  TK_CHECK_ARG(data && weight && attrs && (algos || max_algos <= 0), "null argument");
  ConvGeom g;
  if (conv_geom(data, weight, &attrs->conv, &g) != TK_OK) {
    set_error("tk_conv2d_block_algos: bad shapes");
    return TK_ERR_SHAPE;
  }
  if (!use_mfma_conv(g, attrs->conv.groups) || !is_int8ish(data) || !is_int8ish(weight)) return 0;
  const ConvTraits t = listing_traits(g, weight, attrs);
  int n = 0;
  auto list = [&](int algo) {
    if (n < max_algos) algos[n] = algo;
    ++n;
  };
  // dense blocks (1x1 over [B, K, 1, 1]) with a zero weight zero point: the dense tile kernel first
  if (conv_dense_applies(g, t)) list(kAlgoDense);
  list(kAlgoIm2col);
  n += conv_img_algos(g, &attrs->conv, t, have_chunked(g), algos && max_algos > n ? algos + n : nullptr, max_algos - n);
  // the persistent im2col kernel, last: it measured slower than the im2col kernel on every
  // ResNet-50 layer (profiles/r03w_find_step_pf.json), so the find step's first candidates stay
  // the image-tile plans
  if (conv_pf_applies(g, t)) {
    list(kAlgoPf2);
    list(kAlgoPf3);
  }
  return n;
}

int64_t conv2d_workspace_bytes(const tk_tensor* data, const tk_tensor* weight, const tk_conv2d_attrs* a) {
  if (!a) return -1;
  ConvGeom g;
  if (conv_geom(data, weight, a, &g) != TK_OK) return -1;
  if (!use_mfma_conv(g, a->groups)) return 0;
  return conv_workspace(g, conv_packed_weight_bytes(weight, 1), conv_shadow_bytes(data),
                        conv_scratch_bytes(data, weight, a, 0)).bytes;
}

int conv2d_impl(const tk_tensor* data, const tk_tensor* weight, tk_tensor* out, const tk_conv2d_attrs* a,
                void* workspace, hipStream_t s) {
  TK_CHECK_ARG(data && weight && out && a, "null argument");
  ConvGeom g;
  if (conv_geom(data, weight, a, &g) != TK_OK) {
    set_error("tk_qnn_conv2d: bad shapes");
    return TK_ERR_SHAPE;
  }
  if (!use_mfma_conv(g, a->groups))
    return conv2d_run(data, nullptr, weight, nullptr, nullptr, out, a, nullptr, nullptr, s);
  TK_CHECK_ARG(workspace, "workspace required (tk_qnn_conv2d_workspace_bytes)");
  const ConvWorkspace w = conv_workspace(g, conv_packed_weight_bytes(weight, 1), conv_shadow_bytes(data), 0);
  char* ws = (char*)workspace;
  int32_t* sums = (int32_t*)(ws + w.sums);
  int rc = conv_pack_weight(weight, 1, ws + w.packed, sums, s);
  if (rc) return rc;
  rc = make_shadow_impl(data, ws + w.shadow, s);
  if (rc) return rc;
  return conv2d_run(data, ws + w.shadow, weight, ws + w.packed, sums, out, a, ws + w.scratch, nullptr, s);
}

}  // namespace tk
