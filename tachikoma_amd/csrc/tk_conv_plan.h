// The host-side plan of a conv / dense launch: the conv geometry, what a planner may know of a
// block (ConvTraits), the im2col tile plan with the gemm_i8_kernel variant it names, and the layouts
// of the scratch and workspace buffers.  The scratch size, the algo listing and the launch all read
// this one plan.  Host only, no HIP, nothing touches a device: tools/conv_plan_check.cc sweeps it on
// a CPU.
#pragma once

#include <stdint.h>

#include <cstdlib>

#include "tk_tensor.h"

namespace tk {

constexpr int kBK = 64;          // bytes of K per stage
constexpr int kGemmThreads = 256;

// Kernel-selection switches (TK_XCD, TK_RING, TK_FASTEPI, ...) exist for A/B measurements
// only: they are read from the environment in the ablation build (build.py --ablation,
// -DTK_ABLATION_BUILD, loaded by the tools through TK_LIB_PATH).  The product library
// compiles them to their defaults, so no variable on a box changes what it runs.
#ifdef TK_ABLATION_BUILD
static const char* tune_env(const char* name) { return getenv(name); }
#else
static const char* tune_env(const char*) { return nullptr; }
#endif

static int env_int(const char* name, int dflt) {
  const char* e = tune_env(name);
  return e ? atoi(e) : dflt;
}

inline int64_t al256(int64_t v) { return (v + 255) / 256 * 256; }

// ---------------------------------------------------------------- geometry
struct ConvGeom {
  int N, C, H, W, O, KH, KW, OH, OW, cin_pad, k_pad, k_eff, rows_pad;
};

int conv_geom(const tk_tensor* data, const tk_tensor* weight, const tk_conv2d_attrs* a, ConvGeom* g);
// the MFMA kernels (else the direct / depthwise ones)
bool use_mfma_conv(const ConvGeom& g, int groups);

// The requantize modes that admit the mul_hi form of the block tail (tk_block_tail.h); the host's
// fast_epi decision rests on the mode alone, per-axis shifts living on the device.
constexpr bool rq_fast_mode(int mode) { return mode == TK_RQ_AXIS_UPWARD || mode == TK_RQ_TENSOR_UPWARD; }

// ---------------------------------------------------------------- traits
// What a planner may know of a conv besides its geometry.  Built once per call by conv_traits; the
// fast_epi and unitap rules exist only there.
struct ConvTraits {
  bool block;        // a fused block (else the plain conv: only the int32 record)
  bool patch;        // per-pixel patch sums: a non-zero or per-channel kernel zero point
  int32_t zw;        // kernel zero point of the packed (int8) weight
  bool zw_vec;       // per-channel kernel zero points
  bool has_add;      // residual join
  int64_t in_pix;    // N*H*W of the input
  int fast_epi;      // fast block epilogue: 0 off, 1 nontemporal record stores, 2 plain ones
  bool unitap;       // every 64-byte K stage lies in one tap (the lean im2col walk)
  bool shadow;       // the block writes the shadow of its last record
  int shadow_cpad;   // ... of this many channels
};
// `blk` is the block's attrs; NULL with block = true is a block of which only the conv is known (the
// scratch size is asked that way: no step of the im2col plan reads the tail).
ConvTraits conv_traits(const ConvGeom& g, bool weight_u8, const tk_conv2d_attrs& a, bool block,
                       const tk_block_attrs* blk, bool shadow);

// ---------------------------------------------------------------- gemm_i8_kernel variants
// The instantiations of gemm_i8_kernel that exist, as (MT, im2col, block, mode, ring, wide, BN):
// tk_gemm.hip builds its launch table from this list, the plans name their kernels by these keys.
// mode: 0 whole K + epilogue, 1 split-K partial, 2 split-K reduce + epilogue.  Ring depths 4 and 5
// are A/B variants of the ablation build (ring_depth() is 3 in the product library).
#ifdef TK_ABLATION_BUILD
#define TK_GEMM_RING_VARIANTS(X)                                                                            \
  X(1, true, false, 1, 4, false, 128) X(1, true, false, 1, 5, false, 128) X(1, true, true, 0, 4, true, 128) \
  X(1, true, true, 0, 5, true, 128) X(1, true, true, 0, 4, false, 128) X(1, true, true, 0, 5, false, 128)
#else
#define TK_GEMM_RING_VARIANTS(X)
#endif
#define TK_GEMM_VARIANTS(X)                                                                                  \
  /* conv, split K: partial (plain / wide stages), reduce (plain conv / block) */                             \
  X(1, true, false, 1, 3, false, 128) X(1, true, false, 1, 3, true, 128) X(1, true, false, 2, 3, false, 128)  \
  X(1, true, true, 2, 3, false, 128)                                                                         \
  /* conv blocks, 256-column tiles */                                                                        \
  X(1, true, true, 0, 3, false, 256) X(1, true, true, 0, 3, true, 256)                                       \
  /* conv, 64-row tiles */                                                                                   \
  X(1, true, true, 0, 3, false, 128) X(1, true, true, 0, 3, true, 128) X(1, true, false, 0, 3, false, 128)   \
  /* conv, 128-row tiles */                                                                                  \
  X(2, true, true, 0, 3, false, 128) X(2, true, true, 0, 3, true, 128) X(2, true, false, 0, 3, false, 128)   \
  /* dense */                                                                                                \
  X(2, false, false, 0, 3, false, 128) X(2, false, true, 0, 3, false, 128) X(2, false, false, 1, 3, false, 128) \
  X(2, false, false, 2, 3, false, 128) X(2, false, true, 2, 3, false, 128)                                   \
  TK_GEMM_RING_VARIANTS(X)

struct GemmVariant {
  int mt;
  bool im2col, block;
  int mode, ring;
  bool wide;
  int bn;
  constexpr bool operator==(const GemmVariant& o) const {
    return mt == o.mt && im2col == o.im2col && block == o.block && mode == o.mode && ring == o.ring &&
           wide == o.wide && bn == o.bn;
  }
};
#define TK_GEMM_KEY(MT, IM, BLK, MODE, RING, WIDE, BN) GemmVariant{MT, IM, BLK, MODE, RING, WIDE, BN},
constexpr GemmVariant kGemmVariants[] = {TK_GEMM_VARIANTS(TK_GEMM_KEY)};
#undef TK_GEMM_KEY
constexpr bool gemm_variant_exists(const GemmVariant& v) {
  for (const GemmVariant& k : kGemmVariants)
    if (k == v) return true;
  return false;
}

// ---------------------------------------------------------------- the im2col tile plan
struct Im2colPlan {
  int mt;       // 64-row tiles per workgroup: 1 | 2
  int bn;       // tile columns: 128 | 256
  bool wide;    // 128-byte K stages
  int ring;     // LDS-DMA stages of the main kernel
  int ipt;      // whole images per N tile (0: tiles over the flattened pixel axis)
  int tcols;    // columns of a tile in use
  int32_t ntiles, ntiles8, mtiles;
  int splits, kper;       // split K: kper k-steps (of 64 or 128 bytes) per split
  int64_t partial_bytes;  // the split's partial tiles (0 without a split)
  GemmVariant main, reduce;  // the launch (mode 1 of a split) and the split's reduce (mode 2)
};
Im2colPlan im2col_plan(const ConvGeom& g, const ConvTraits& t);

// ---------------------------------------------------------------- layouts
// Scratch of an MFMA conv: the patch sums, then one region shared by whichever kernel runs -- the
// im2col split's partial tiles, or `other_bytes` (the image-tile split plans' partial records and
// the dense head's K-slice sums, which their own files size).
struct ConvScratch {
  int64_t patch, partials, bytes;  // offsets of the two regions; total
};
ConvScratch conv_scratch(const ConvGeom& g, const ConvTraits& t, const Im2colPlan& p, int64_t other_bytes);

// Workspace of the one-call tk_qnn_conv2d: packed weight, weight sums, shadow, scratch.
struct ConvWorkspace {
  int64_t packed, sums, shadow, scratch, bytes;
};
ConvWorkspace conv_workspace(const ConvGeom& g, int64_t packed_bytes, int64_t shadow_bytes, int64_t scratch_bytes);

// A dense GEMM on 128 x 128 tiles: the split and the workspace (padded operands, their row sums,
// the split's partial tiles).
struct DensePlan {
  int k_pad, mrows, nrows;
  int32_t ntiles, ntiles8, mtiles;
  int splits, kper;
  int64_t pad_a, pad_b, sum_a, sum_b, partials, bytes;  // offsets; total
  GemmVariant main, reduce;
};
DensePlan dense_plan(int64_t M, int64_t N, int64_t K, bool block);

}  // namespace tk
