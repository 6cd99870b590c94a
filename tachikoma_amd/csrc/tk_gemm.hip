// int8 x int8 -> int32 contractions on the gfx950 matrix cores.
//
// qnn.conv2d is an implicit GEMM   C[cout][p] = Σ_k W'[cout][k] · X'[p][k]
// and qnn.dense a plain GEMM        C[m][n]    = Σ_k D'[m][k]   · W'[n][k]
// both computed by one MFMA kernel (v_mfma_i32_32x32x32_i8) over operands whose
// reduction axis is contiguous:
//   * weights are packed once to [Cout][KH][KW][Cin_pad] (Cin_pad = Cin rounded
//     to 16, K rounded to 64; padding bytes are 0, uint8 stored xor 0x80),
//   * conv activations are read from a channel-blocked int8 "shadow" of the NCHW tensor,
//     gathered per 16-byte chunk (one tap, 16 channels) straight into LDS.
// The zero points are folded exactly (modulo 2^32, like the reference's int32
// accumulation) with row sums:
//   Σ(a-za)(w-zw) = Σ a'w - za·Σw - zw·Σa' + K·za·zw
// where out-of-bounds taps hold a' = za on real channels (they contribute 0,
// python/tvm/relay/qnn/op/legalizations.py:195-226 pads with zeros after the shift).
// The epilogue writes int32 NCHW directly (lanes run along pixels: coalesced).
//
// This file holds gemm_i8_kernel, the table from a variant key (tk_conv_plan.h) to its
// instantiation, and the dense path.  The conv host code is tk_conv.cc, operand preparation
// tk_conv_prep.hip.
#include <algorithm>
#include <string>
#include <type_traits>

#include "tk_conv.h"
#include "tk_ops.h"

namespace tk {

// V consecutive columns of one row after zero-point folding: stores each record as
// soon as it is complete, transforming v in place (conv → bias_add → requantize →
// [qnn.add] → [clip], tk_block_tail.h).  The channel is the row (conv blocks: constants r)
// or the column (dense blocks: constants cc[q], loaded once per thread with block_consts).
template <int V, bool kBlock>
__device__ __forceinline__ void epi_apply(const GemmArgs& g, const EpiRow& r, int32_t* v, int64_t off, bool st,
                                          int col, uint32_t resid, const int32_t* lut, const BlockConsts* cc) {
  if (st && !(g.ablate & 8)) st_i32<V>(g.C + off, v, g.nt);
  if (!kBlock) return;
  const int32_t qmin = (int32_t)g.rq.qmin, qmax = (int32_t)g.rq.qmax, zpo = g.rq.zp_out;
  const int mode = g.rq.mode;
#pragma unroll
  for (int q = 0; q < V; ++q) v[q] = (int32_t)((uint32_t)v[q] + (uint32_t)(g.ch_is_row ? r.bias : cc[q].bias));
  if (st && !(g.ablate & 16)) st_i32<V>(g.bias_out + off, v, g.nt);
  if (!g.ch_is_row) {
#pragma unroll
    for (int q = 0; q < V; ++q) v[q] = block_rq<false>((uint32_t)v[q], (uint32_t)cc[q].zp, cc[q].m, cc[q].s, mode, zpo, qmin, qmax);
  } else if (block_rq_fast_ok(mode, r.s)) {
#pragma unroll
    for (int q = 0; q < V; ++q) v[q] = block_rq<true>((uint32_t)v[q], (uint32_t)r.zp, r.m, r.s, mode, zpo, qmin, qmax);
  } else {
#pragma unroll
    for (int q = 0; q < V; ++q) v[q] = block_rq<false>((uint32_t)v[q], (uint32_t)r.zp, r.m, r.s, mode, zpo, qmin, qmax);
  }
  if (st && !(g.ablate & 32)) st_i8<V>(g.rq_out + off, v, g.nt);
  if (g.has_add) {
#pragma unroll
    for (int q = 0; q < V; ++q) v[q] = block_join(v[q], (resid >> (8 * q)) & 0xFFu, lut, g.add_zp, qmin, qmax);
    if (st) st_i8<V>(g.add_out + off, v, g.nt);
  }
  if (g.has_clip) {
#pragma unroll
    for (int q = 0; q < V; ++q) v[q] = block_clip(v[q], g.clip_lo, g.clip_hi);
    if (st && !(g.ablate & 64)) st_i8<V>(g.clip_out + off, v, g.nt);
  }
}


// LDS tile [rows][64 B], 16-byte chunk c of row r stored at chunk c ^ ((r >> 2) & 3):
// the 16-lane groups of ds_read_b128 then hit 16 distinct bank slots.
__device__ __forceinline__ int lds_off(int row, int chunk) { return row * kBK + ((chunk ^ ((row >> 2) & 3)) << 4); }

// Same for stages of SBK = 64 or 128 bytes per row.  128-byte rows: chunk c of row r at
// chunk c ^ ((r >> 1) & 7) (two rows per 256-byte bank period, 8 row pairs per 16 lanes).
template <int SBK>
__device__ __forceinline__ int lds_off_w(int row, int chunk) {
  if constexpr (SBK == 64) return lds_off(row, chunk);
  else return row * SBK + ((chunk ^ ((row >> 1) & 7)) << 4);
}


// XCD-aware tile order: workgroup L runs on XCD L % 8, so XCD x takes the N tiles x, x+8,
// x+16, ... and for each of them all M tiles back to back: the workgroups that share an
// N tile (the same im2col B rows) run close together on one XCD and hit its L2.
__device__ __forceinline__ void tile_of(const GemmArgs& g, int& mt, int& nt) {
  const int L = blockIdx.x;
  if (!g.xcd_order) {  // plain order (N tiles fastest), for A/B measurements
    mt = L / g.ntiles8;
    nt = L - mt * g.ntiles8;
    return;
  }
  const int local = L >> 3;
  mt = local % g.mtiles;
  if (g.xcd_order == 2) {  // contiguous N-tile chunks per XCD (A/B: adjacent tiles share an L2)
    nt = (L & 7) * (g.ntiles8 >> 3) + local / g.mtiles;
    return;
  }
  nt = (local / g.mtiles) * 8 + (L & 7);
}

// kMode: 0 = whole K + epilogue; 1 = split-K partial (raw accumulators to g.ws);
//        2 = sum the split-K partials of this tile + epilogue (no main loop).


// kWide (im2col LDS-DMA path): 128-byte K stages instead of 64, i.e. half the
// barrier-separated steps of long reductions (each step pays a fixed LDS / barrier / address
// latency that the 1-2 workgroups per CU of the small-grid layers cannot hide).
// BN = 256 (image tiles of 65..256 pixels, conv blocks only): each wave owns 4 32-col tiles, and a
// tile's 64 channels x one image are one contiguous run of every NCHW record (see the flat
// epilogue): on 14x14 planes such runs store 2x faster than 128-column tiles that cross images
// (tools/probe_store3.hip, profiles/r02j_store_patterns.txt).
template <int MT, bool kIm2col, bool kBlock, int kMode = 0, int kRing = 3, bool kWide = false, int BN = 128>
__global__ __launch_bounds__(kGemmThreads, BN == 256 ? (kWide ? 1 : 2)
                                           : MT == 1 ? (kWide ? (kRing == 3 ? 2 : 1) : kRing == 3 ? 4 : kRing == 4 ? 3 : 2)
                                                     : (kWide ? 1 : 2)) void
gemm_i8_kernel(GemmArgs g) {
  static_assert(!kWide || (kIm2col && (MT == 1 || (kBlock && kMode == 0 && kRing == 3))), "wide stages: im2col");
  static_assert(BN == 128 || (BN == 256 && MT == 1 && kIm2col && kBlock && kMode == 0), "256-column tiles: conv blocks");
  constexpr int BM = 64 * MT;   // rows of A per block (2 waves along M, MT 32-row tiles each)
  constexpr int NJ = BN / 64;   // 32-col tiles per wave (2 waves along N)
  constexpr int kStr = BN + 4;  // dwords per LDS row of the epilogue tile (breaks the 64-bank period)
  constexpr int kFlat = BM * BN / 1024;  // 4-element groups per thread of the flat epilogue
  // 4-column epilogues: kLPR lanes per tile row (4 columns each), kRPI rows per pass, kRows passes
  constexpr int kLPR = BN / 4, kRPI = kGemmThreads / kLPR, kRows = BM / kRPI;
  constexpr int A_CHUNKS = BM * kBK / 16 / kGemmThreads;  // 16-byte loads per thread per stage (plain path)
  constexpr int B_CHUNKS = BN * kBK / 16 / kGemmThreads;
  constexpr int SBK = kWide ? 2 * kBK : kBK;              // K bytes per stage
  constexpr int CPR = SBK / 16;                           // 16-byte chunks per stage row
  constexpr int RPP = kGemmThreads / CPR;                 // stage rows per pass of all threads
  constexpr int A_DMA = BM / RPP, B_DMA = BN / RPP;       // LDS-DMA loads per thread per stage
  constexpr int kStageBytes = (BM + BN) * SBK;
  // kRing: LDS-DMA stages of the im2col path (kRing - 1 in flight); the plain path double-buffers
  constexpr int kStage = (kIm2col ? kRing : 2) * kStageBytes;
  constexpr int kEpi = BM * kStr * 4 + BM * (int)sizeof(EpiRow) + (kBlock ? 512 * 4 + 16 : 0);  // + flat sink slot
  __shared__ __attribute__((aligned(16))) int8_t smem[kStage > kEpi ? kStage : kEpi];
  __shared__ int s_fast;  // tile-uniform: every row's shift admits the mul_hi form (block_rq_fast_shift)
  int8_t* As = smem;
  int8_t* Bs = smem + 2 * BM * kBK;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  [[maybe_unused]] const int abl = g.ablate;
  if (kBlock && tid == 0) s_fast = 1;  // visible after the first barrier; only cleared later
  int mtile, ntile;
  tile_of(g, mtile, ntile);
  if (ntile >= g.ntiles) return;  // padding of the N-tile count to a multiple of 8
  const int m0 = mtile * BM;
  const int n0 = ntile * g.tcols;
  // per-row epilogue constants (threads < BM, one row each), loaded up front: they land
  // during the main loop
  // (raw loads from a dummy word where an array is absent: the per-row/scalar choice is
  // made at the epilogue, so no path waits for the loads here)
  EpiRow row_pre{};
  const bool rq_axis = g.rq.mode >= TK_RQ_AXIS_UPWARD;
  if (kMode != 1 && tid < BM) {
    const int row = min(m0 + tid, g.M - 1);
    auto raw = [&](const int32_t* p, bool use) { return ldg(use ? p + row : tk_zero_words); };
    row_pre.ra = (uint32_t)raw(g.RA, g.RA != nullptr);
    row_pre.za = (uint32_t)raw(g.zA_vec, g.zA_vec != nullptr);
    if (kBlock && g.ch_is_row) {
      row_pre.bias = raw(g.bias, true);
      row_pre.m = raw(g.rq.ms, rq_axis);
      row_pre.s = raw(g.rq.ss, rq_axis);
      row_pre.zp = raw(g.rq.zps, g.rq.zps != nullptr);
    }
  }
  // residual bytes of every row this thread writes (4-column and flat epilogue paths).  kNR
  // loads, every one issued (a thread with nothing to join reads the zero words), so that the
  // counted waits below know them: on the LDS-DMA path they go out right after the prologue's
  // stages -- the stage waits let them stay in flight, the epilogue stores its conv / bias_add /
  // requantize records before it needs them -- because in the network the residual is a record
  // written several kernels earlier and comes from HBM behind the CU's stores (the 56x56
  // expands ran 115 us with a cached residual and 153 us with a cold one, r05w); elsewhere
  // they are issued here, before the main loop.
  static_assert(kFlat == kRows, "one residual word per 4-element group");
  constexpr int kNR = kBlock && kMode != 1 ? kFlat : 0;
  constexpr bool kLateResid = kNR > 0 && kIm2col && kMode != 2;
  uint32_t resid_pre[kFlat > kRows ? kFlat : kRows];
  auto issue_resid = [&]() __attribute__((always_inline)) {
    if constexpr (kNR > 0) {
      const uint32_t* zw = reinterpret_cast<const uint32_t*>(tk_zero_words);
      const int hw = g.OH * g.OW;
      if (g.has_add && g.ipt) {
        // flat epilogue: 4 consecutive elements of an image run per group (see there)
        const int run = min(BM, g.M - m0) * hw;
#pragma unroll
        for (int k = 0; k < kFlat; ++k) {
          const int gi = tid + kGemmThreads * k;
          const int kk = gi / (16 * hw), f = (gi - kk * 16 * hw) * 4;
          const int img = n0 / hw + kk;
          const bool ok = kk < g.ipt && img < g.N / hw && f < run;
          resid_pre[k] = ldg(ok ? reinterpret_cast<const uint32_t*>(g.add_res + ((int64_t)img * g.M + m0) * hw + f) : zw);
        }
      } else if (g.has_add && g.vecw >= 4) {
        const int col = n0 + (tid % kLPR) * 4;
        const int img = col / hw;
        const int64_t cbase = (int64_t)img * g.M * hw + (col - img * hw);
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
          const int row = m0 + tid / kLPR + kRPI * k;
          const bool ok = col < g.N && row < g.M;
          resid_pre[k] = ldg(reinterpret_cast<const uint32_t*>(g.add_res + (ok ? cbase + (int64_t)row * hw : 0)));
        }
      } else {
#pragma unroll
        for (int k = 0; k < kNR; ++k) resid_pre[k] = ldg(zw);
      }
    }
  };
  if constexpr (!kLateResid) issue_resid();
  const int kc = tid & 3;  // this thread's 16-byte chunk within a K stage

  // ---- per-thread im2col state for the B rows it loads
  int b_img[B_DMA], b_ih0[B_DMA], b_iw0[B_DMA];
  bool b_valid[B_DMA];
#pragma unroll
  for (int t = 0; t < B_DMA; ++t) {
    int row = tid / CPR + t * RPP;
    int p = n0 + row;
    b_valid[t] = p < g.N && row < g.tcols;
    if (kIm2col) {
      const uint32_t pp = b_valid[t] ? p : 0;
      const int hw = g.OH * g.OW;
      const int img = g.mg_hw ? (int)(((uint64_t)pp * g.mg_hw) >> 40) : (int)(pp / (uint32_t)hw);
      const uint32_t rem = pp - img * hw;
      const int oh = g.mg_ow ? (int)(((uint64_t)rem * g.mg_ow) >> 40) : (int)(rem / (uint32_t)g.OW);
      const int ow = rem - oh * g.OW;
      b_img[t] = img;
      b_ih0[t] = oh * g.sh - g.pt;
      b_iw0[t] = ow * g.sw - g.pl;
    }
  }

  v4i ra[A_CHUNKS], rb[B_CHUNKS];

  auto load_stage = [&](int k0) {
#pragma unroll
    for (int t = 0; t < A_CHUNKS; ++t) {
      int row = (tid >> 2) + t * (kGemmThreads / 4);
      ra[t] = *reinterpret_cast<const v4i*>(g.A + (int64_t)(m0 + row) * g.lda + k0 + kc * 16);
    }
#pragma unroll
    for (int t = 0; t < B_CHUNKS; ++t) {
      int row = (tid >> 2) + t * (kGemmThreads / 4);
      rb[t] = *reinterpret_cast<const v4i*>(g.B + (int64_t)(n0 + row) * g.ldb + k0 + kc * 16);
    }
  };

  auto store_stage = [&](int buf) {
    int8_t* a = As + buf * BM * kBK;
    int8_t* b = Bs + buf * BN * kBK;
#pragma unroll
    for (int t = 0; t < A_CHUNKS; ++t) {
      int row = (tid >> 2) + t * (kGemmThreads / 4);
      *reinterpret_cast<v4i*>(a + lds_off(row, kc)) = ra[t];
    }
#pragma unroll
    for (int t = 0; t < B_CHUNKS; ++t) {
      int row = (tid >> 2) + t * (kGemmThreads / 4);
      *reinterpret_cast<v4i*>(b + lds_off(row, kc)) = rb[t];
    }
  };

  v16i acc[MT][NJ];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = v16i{0};

  // partial tiles live in g.ws in register order: v4i r4 of fragment (i, j) of thread tid
  constexpr int kTileInts = MT * 2 * 16 * kGemmThreads;
  const int64_t tile = (int64_t)mtile * g.ntiles + ntile;
  if constexpr (kMode == 2) {
    // sum the partial tiles; two splits' loads are issued together (MT = 1: 16 x 16 B
    // in flight per lane) so the reduction pays the L2 latency once per pair
    constexpr int kPair = MT == 1 ? 2 : 1;
    auto add_tile = [&](const v4i* t) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const v4i u = t[(i * 2 + j) * 4 + r4];
            acc[i][j][4 * r4] += u.x;
            acc[i][j][4 * r4 + 1] += u.y;
            acc[i][j][4 * r4 + 2] += u.z;
            acc[i][j][4 * r4 + 3] += u.w;
          }
    };
    int sp = 0;
    for (; sp + kPair <= g.splits; sp += kPair) {
      v4i t[kPair][MT * 2 * 4];
#pragma unroll
      for (int p = 0; p < kPair; ++p) {
        const v4i* src = reinterpret_cast<const v4i*>(g.ws + (tile * g.splits + sp + p) * kTileInts);
#pragma unroll
        for (int f = 0; f < MT * 2 * 4; ++f) t[p][f] = src[f * kGemmThreads + tid];
      }
#pragma unroll
      for (int p = 0; p < kPair; ++p) add_tile(t[p]);
    }
    for (; sp < g.splits; ++sp) {
      const v4i* src = reinterpret_cast<const v4i*>(g.ws + (tile * g.splits + sp) * kTileInts);
      v4i t[MT * 2 * 4];
#pragma unroll
      for (int f = 0; f < MT * 2 * 4; ++f) t[f] = src[f * kGemmThreads + tid];
      add_tile(t);
    }
  }
  int kt0 = 0, nk = g.k_pad / SBK;
  if constexpr (kMode == 1) {
    kt0 = blockIdx.z * g.kper;
    nk = min(nk, kt0 + g.kper);
  }
  // MFMAs of one staged K step (2 x K=32) from LDS
  // every fragment of the stage is read before the first MFMA: one LDS round trip per
  // stage instead of one per K=32 half (small grids run 1-2 workgroups per CU, so the
  // LDS latency is not hidden by other waves)
  constexpr int KS = SBK / 32;  // K = 32 MFMA steps per stage
  struct Frags {
    v4i a[KS][MT], b[KS][NJ];
  };
  auto read_frags = [&](const int8_t* a, const int8_t* b, Frags& f) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int chunk = 2 * ks + (lane >> 5);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        int row = wm * 32 * MT + i * 32 + (lane & 31);
        f.a[ks][i] = *reinterpret_cast<const v4i*>(a + lds_off_w<SBK>(row, chunk));
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        int row = wn * (BN / 2) + j * 32 + (lane & 31);
        f.b[ks][j] = *reinterpret_cast<const v4i*>(b + lds_off_w<SBK>(row, chunk));
      }
    }
  };
  auto mfma_frags = [&](const Frags& f) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(f.a[ks][i], f.b[ks][j], acc[i][j], 0, 0, 0);
  };
  auto mma_stage = [&](const int8_t* a, const int8_t* b) {
    Frags f;
    read_frags(a, b, f);
    __builtin_amdgcn_sched_barrier(0);  // keep the reads ahead of the MFMAs (the scheduler interleaves them)
    mfma_frags(f);
  };

  if constexpr (kMode != 2 && kIm2col) {
#ifdef TK_ABLATION_BUILD
    const int ablate = __builtin_amdgcn_readfirstlane(g.ablate);  // profiling builds only
#else
    constexpr int ablate = 0;  // the main-loop ablation branches compile away
#endif
    // ---- LDS-DMA pipeline (conv): a kRing-stage ring filled by global_load_lds_dwordx4 with
    // kRing - 1 stages in flight across the barrier (counted vmcnt + raw s_barrier).
    // The LDS image is lane-linear (lane l of a wave-instruction lands at base + 16 l =
    // row l/4, slot l%4), so the bank swizzle of lds_off goes on the SOURCE: slot s of row r
    // holds chunk s ^ ((r >> 2) & 3), i.e. lane l loads chunk (l & 3) ^ ((l >> 4) & 3).
    // Out-of-bounds taps read a row of the input zero point; rows past N and K padding
    // (whose weights are 0) read it too.
    // (wide: 8 rows of 128 B per wave-instruction, slot s of row r holds chunk s ^ ((r >> 1) & 7))
    const int cl = kWide ? ((lane & 7) ^ ((4 * wave + (lane >> 4)) & 7)) : ((lane & 3) ^ ((lane >> 4) & 3));
    const int8_t* fill_src = reinterpret_cast<const int8_t*>(tk_fill_rows.v + 16 * (g.fill & 0xFFu));
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int8_t* a_src[A_DMA];
#pragma unroll
    for (int t = 0; t < A_DMA; ++t)
      a_src[t] = g.A + (int64_t)(m0 + tid / CPR + t * RPP) * g.lda + kt0 * SBK + cl * 16;
    const int nst = nk - kt0;
    auto pipeline = [&](auto&& issue) {
#pragma unroll
      for (int st = 0; st < kRing - 1; ++st)
        if (st < nst) issue(st);
      if constexpr (kLateResid) {
        // younger than the prologue's stages (see there): the counted stage waits below let the
        // kNR residual loads stay in flight only if they are issued after every prologue DMA, so
        // the scheduler may not move them across (the plain loads and the LDS-DMAs are otherwise
        // independent to it)
        __builtin_amdgcn_sched_barrier(0);
        issue_resid();
        __builtin_amdgcn_sched_barrier(0);
      }
      int cur = 0, nxt = kRing - 1;  // ring slots of stage it and of stage it + kRing - 1
      // one step: retire stage it (A_DMA + B_DMA LDS-DMAs per thread and stage) with `pending`
      // later stages still in flight, barrier (stage it visible to all waves; the slot read in
      // step it-1 is free), fragments of stage it first so that their LDS latency overlaps the
      // next issue, then the MFMAs
      // extra: the residual loads still allowed in flight (steps retiring a prologue stage)
      auto step = [&](int it, int pending, int extra) __attribute__((always_inline)) {
        if (extra) wait_vm_any(pending * (A_DMA + B_DMA) + extra);
        else wait_vm(pending * (A_DMA + B_DMA));
        if (ablate & 4096) {
        } else if (ablate & 1024) asm volatile("s_barrier" ::: "memory");
        else lds_barrier();
        const int8_t* a = smem + cur * kStageBytes;
        Frags f;
        if (!(ablate & 2048)) read_frags(a, a + BM * SBK, f);
        __builtin_amdgcn_sched_barrier(0);
        if (it + kRing - 1 < nst) {
          issue(nxt);
          nxt = nxt == kRing - 1 ? 0 : nxt + 1;
        }
        __builtin_amdgcn_sched_barrier(0);
        if (!(ablate & 512)) mfma_frags(f);
        cur = cur == kRing - 1 ? 0 : cur + 1;
      };
      // steady state with a compile-time wait count, then the last kRing - 2 stages
      const int steady = nst - (kRing - 2);
      constexpr int kLate = kLateResid ? kNR : 0;
      int it = 0;
      for (; it < steady && it < kRing - 1; ++it) step(it, kRing - 2, kLate);
      for (; it < steady; ++it) step(it, kRing - 2, 0);
      for (; it < nst; ++it) step(it, nst - 1 - it, it < kRing - 1 ? kLate : 0);
    };
    auto issue_a = [&](int8_t* sa) {
#pragma unroll
      for (int t = 0; t < A_DMA; ++t) {
        if (!(ablate & 128))
          __builtin_amdgcn_global_load_lds((const void*)a_src[t], (void*)(sa + ((RPP / 4) * wave_u + RPP * t) * SBK),
                                           16, 0, 0);
        a_src[t] += SBK;
      }
    };
    if (kWide || g.unitap) {
      // lane-constant part of the source (pixel + the lane's channel group) and the taps
      // that are in bounds for the lane's rows; the stage part (channel group, tap) is uniform
      const int8_t* lane_base[B_DMA];
      uint64_t tmask[B_DMA];
#pragma unroll
      for (int t = 0; t < B_DMA; ++t) {
        const int64_t pix = ((int64_t)b_img[t] * g.H + b_ih0[t]) * g.W + b_iw0[t];
        lane_base[t] = g.B + (pix + (int64_t)cl * g.in_pix) * 16;
        uint32_t rows = 0, cols = 0;
        for (int kh = 0; kh < g.KH; ++kh) {
          const int ih = b_ih0[t] + kh * g.dh;
          rows |= (uint32_t)(ih >= 0 && ih < g.H) << kh;
        }
        for (int kw = 0; kw < g.KW; ++kw) {
          const int iw = b_iw0[t] + kw * g.dw;
          cols |= (uint32_t)(iw >= 0 && iw < g.W) << kw;
        }
        uint64_t m = 0;
        for (int kh = 0; kh < g.KH; ++kh)
          if ((rows >> kh) & 1) m |= (uint64_t)cols << (kh * g.KW);
        tmask[t] = b_valid[t] ? m : 0;
      }
      int cg, kh, kw;  // uniform: channel group of the stage's first chunk, tap
      {
        const int k0 = kt0 * SBK;
        const int tap = k0 / g.cin_pad;
        cg = (k0 - tap * g.cin_pad) >> 4;
        kh = tap / g.KW;
        kw = tap - kh * g.KW;
      }
      const int64_t grp_bytes = g.in_pix * 16;
      const int64_t row_bytes = (int64_t)g.dh * g.W * 16;
      const int KW = g.KW, cgroups = g.cgroups, dw16 = g.dw * 16;
      int tap = kh * KW + kw;
      int64_t soff = cg * grp_bytes + kh * row_bytes + (int64_t)kw * dw16;
      pipeline([&](int slot) {
        int8_t* sa = smem + slot * kStageBytes;
        issue_a(sa);
        int8_t* sb = sa + BM * SBK;
        const bool grp_ok = cg + cl < cgroups;  // K padding of a 1x1 conv with cin_pad % 64 != 0
#pragma unroll
        for (int t = 0; t < B_DMA; ++t) {
          const bool ok = ((tmask[t] >> tap) & 1) && grp_ok;
          const int8_t* src = ok ? lane_base[t] + soff : fill_src;
          if (!(ablate & 256))
            __builtin_amdgcn_global_load_lds((const void*)src, (void*)(sb + ((RPP / 4) * wave_u + RPP * t) * SBK),
                                             16, 0, 0);
        }
        cg += CPR;
        soff += CPR * grp_bytes;
        if (cg >= cgroups) {
          cg = 0;
          ++tap;
          if (++kw == KW) kw = 0, ++kh;
          soff = kh * row_bytes + (int64_t)kw * dw16;
        }
      });
    } else if constexpr (!kWide) {
      // general walk: the thread's chunk is (tap, channel offset c0) with the taps in
      // (kh, kw) order; advanced 64 bytes per stage without divisions
      int c0, kh, kw;
      {
        const int kg = kt0 * kBK + cl * 16;
        const int tap = kg / g.cin_pad;
        c0 = kg - tap * g.cin_pad;
        kh = tap / g.KW;
        kw = tap - kh * g.KW;
      }
      int b_pix[B_CHUNKS];
#pragma unroll
      for (int t = 0; t < B_CHUNKS; ++t) b_pix[t] = (b_img[t] * g.H + b_ih0[t]) * g.W + b_iw0[t];
      pipeline([&](int slot) {
        int8_t* sa = smem + slot * kStageBytes;
        issue_a(sa);
        int8_t* sb = sa + BM * kBK;
        const bool tap_ok = kh < g.KH;
        const int dy = kh * g.dh, dx = kw * g.dw;
        const int64_t plane = (int64_t)(c0 >> 4) * g.in_pix;
#pragma unroll
        for (int t = 0; t < B_CHUNKS; ++t) {
          const int ih = b_ih0[t] + dy;
          const int iw = b_iw0[t] + dx;
          const bool inb = ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
          const int8_t* src = g.B + (plane + b_pix[t] + dy * g.W + dx) * 16;
          src = (b_valid[t] && tap_ok && inb) ? src : fill_src;
          if (!(ablate & 256))
            __builtin_amdgcn_global_load_lds((const void*)src, (void*)(sb + (16 * wave_u + 64 * t) * kBK), 16, 0, 0);
        }
        c0 += kBK;
        while (c0 >= g.cin_pad) {
          c0 -= g.cin_pad;
          if (++kw == g.KW) kw = 0, ++kh;
        }
      });
    }
  }
  if constexpr (kMode != 2 && !kIm2col) {
  load_stage(kt0 * kBK);
  store_stage(0);
  __syncthreads();

  for (int kt = kt0; kt < nk; ++kt) {
    const int buf = (kt - kt0) & 1;
    if (kt + 1 < nk) load_stage((kt + 1) * kBK);  // issue early, land under the MFMAs
    mma_stage(As + buf * BM * kBK, Bs + buf * BN * kBK);
    if (kt + 1 < nk) store_stage(buf ^ 1);
    __syncthreads();
  }
  }  // plain path
  // every load issued so far (LDS-DMA stages, the row constants) has landed: a wait the
  // compiler sees (the ring's counted waits are inline asm), so that it does not add
  // conservative vmcnt(0) waits before the epilogue's LDS reads.  The late residual loads (the
  // youngest, see issue_resid) may stay in flight: vmcnt(kNR)
  if constexpr (kLateResid) {
    __builtin_amdgcn_s_waitcnt(0x0F70 | (kNR & 15) | ((kNR >> 4) << 14));
  } else {
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  }
  if constexpr (kMode == 1) {
    v4i* dst = reinterpret_cast<v4i*>(g.ws + (tile * gridDim.z + blockIdx.z) * kTileInts);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
          dst[((i * 2 + j) * 4 + r4) * kGemmThreads + tid] =
              v4i{acc[i][j][4 * r4], acc[i][j][4 * r4 + 1], acc[i][j][4 * r4 + 2], acc[i][j][4 * r4 + 3]};
    return;
  }

  // ---- epilogue: the whole BM x BN accumulator tile is staged through LDS.
  //  (1) every wave dumps its raw accumulators to LDS [row][col]; threads < BM stage their
  //      row's constants (bias, multiplier, shift, zero points, fold term) next to it;
  //  (2) every thread owns fixed columns (4 consecutive ones when the plane length is a
  //      multiple of 4, else 1) and walks rows: per row, zero-point folding, then each record
  //      is stored as soon as it is complete.  The lanes of a wave run along the columns, so
  //      every store instruction writes whole 128-byte lines of one or two rows (int32: 16 B
  //      per lane, int8: 4 B per lane); the final int8 values go back to the LDS slot;
  //  (3) the shadow for the next conv: each item gathers 16 channels of one pixel (a wave
  //      reads 64 consecutive columns per row: conflict-free) into a 16 B store; the lanes'
  //      stores are contiguous (channel-blocked layout).
  if (g.ablate & 4) return;
  int32_t* tileI = reinterpret_cast<int32_t*>(smem);
  EpiRow* rowc = reinterpret_cast<EpiRow*>(smem + BM * kStr * 4);
  int32_t* lut = reinterpret_cast<int32_t*>(smem + BM * kStr * 4 + BM * sizeof(EpiRow));  // [2][256]
  const int hw = g.OH * g.OW;
  const bool zb_vec = g.zB_vec != nullptr, has_rb = g.RB != nullptr;
  const bool simple_fold = !zb_vec && !has_rb;
  lds_barrier();  // staging buffers are free
  if (tid < BM) {
    EpiRow r = row_pre;
    if (!g.RA) r.ra = 0;
    if (!g.zA_vec) r.za = (uint32_t)g.zA;
    if (kBlock && g.ch_is_row) {
      if (!rq_axis) r.m = g.rq.multiplier, r.s = g.rq.shift;
      if (!g.rq.zps) r.zp = g.rq.zp_in;
    }
    r.fold = (uint32_t)g.k_eff * r.za * (uint32_t)g.zB - (uint32_t)g.zB * r.ra;
    if (kBlock && g.ch_is_row && !block_rq_fast_shift(r.s)) s_fast = 0;
    rowc[tid] = r;
  }
  if (kBlock && g.has_add) {
    block_join_lut(tid, lut, g.rq.qmin == 0, g.add_up_b, g.add_up_r, g.add_pb, g.add_pr);
  }
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int lc = wn * (BN / 2) + j * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int lr = wm * 32 * MT + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        tileI[lr * kStr + lc] = acc[i][j][r];
      }
    }
  }
  lds_barrier();

  bool done = false;
  if constexpr (kBlock) {
    if (g.ipt && (BN == 256 || !(g.ablate & 0x7F))) {
      // ---- flat epilogue (image-aligned tiles, planes of 1..64 pixels): for image kk of the
      // tile, its channels m0.. and all OH*OW pixels are one contiguous run of the NCHW
      // records, `run` elements long.  Group gi = 4 consecutive elements of one run: b128
      // stores of the int32 records and b32 stores of the 8-bit ones, contiguous across lanes
      // (whole 128-byte lines), each element gathered from its (row, column) slot of the tile.
      done = true;
      const int run = min(BM, g.M - m0) * hw;
      const int img0 = n0 / hw, nimg = g.N / hw;
      const uint32_t n4 = g.out_elems * 4u;
      const auto r_conv = rec_rsrc(g.C, n4), r_bias = rec_rsrc(g.bias_out, n4);
      const auto r_rq = rec_rsrc(g.rq_out, g.out_elems);
      const auto r_add = rec_rsrc(g.add_out, g.has_add ? g.out_elems : 0u);
      const auto r_clip = rec_rsrc(g.clip_out, g.has_clip ? g.out_elems : 0u);
      const int32_t qmin = (int32_t)g.rq.qmin, qmax = (int32_t)g.rq.qmax, zpo = g.rq.zp_out;
      const int32_t add_zp = g.add_zp, clip_lo = g.clip_lo, clip_hi = g.clip_hi;
      const bool has_add = g.has_add, has_clip = g.has_clip;
      const int mode = g.rq.mode;
      const int ipt = g.ipt, Mrows = g.M;  // (the lambda must not reference g: that forces it to scratch)
      // x / hw as (x * mg) >> 40, exact for x * hw < 2^40 (x here < 2^16)
      const uint64_t mg = ((1ull << 40) + (uint64_t)hw - 1) / (uint64_t)hw;
      auto groups = [&](auto fast_c, auto rowu_c) __attribute__((always_inline)) {
        constexpr bool FAST = decltype(fast_c)::value;
        // ROWU (hw % 4 == 0): a group's 4 elements lie in one row, 16-byte aligned in LDS: one
        // b128 read of the tile, one row of constants
        constexpr bool ROWU = decltype(rowu_c)::value;
#pragma unroll
        for (int k = 0; k < kFlat; ++k) {
          const int gi = tid + kGemmThreads * k;
          const int kk = (int)((((uint64_t)(gi >> 4)) * mg) >> 40), f = (gi - kk * 16 * hw) * 4;
          if (!(kk < ipt && img0 + kk < nimg && f < run)) continue;  // past a run or the tile's images
          const uint32_t o = (uint32_t)(((img0 + kk) * Mrows + m0) * hw + f);
          const int r0 = (int)(((uint64_t)f * mg) >> 40), p0 = f - r0 * hw;
          int slot[4];
          EpiRow rr[4];
          v4u v;
          if constexpr (ROWU) {
            slot[0] = r0 * kStr + kk * hw + p0;
            rr[0] = rowc[r0];
#pragma unroll
            for (int e = 1; e < 4; ++e) slot[e] = slot[0] + e, rr[e] = rr[0];
            v = *reinterpret_cast<const v4u*>(tileI + slot[0]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              int re = r0, pe = p0 + e;
#pragma unroll
              for (int w = 0; w < 3; ++w)  // one row change per group when hw >= 4, up to 3 below
                if (pe >= hw) pe -= hw, ++re;
              slot[e] = re * kStr + kk * hw + pe;
              rr[e] = rowc[re];
              v[e] = (uint32_t)tileI[slot[e]];
            }
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += rr[e].fold;
          if (!TK_ABL(2)) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i, v), r_conv, o * 4u, 0, kAuxNT);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += (uint32_t)rr[e].bias;
          if (!TK_ABL(2)) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i, v), r_bias, o * 4u, 0, kAuxNT);
          int32_t q[4];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            q[e] = block_rq<FAST>(v[e], (uint32_t)rr[e].zp, rr[e].m, rr[e].s, mode, zpo, qmin, qmax);
          if (!TK_ABL(2)) __builtin_amdgcn_raw_buffer_store_b32(pack4u(q[0], q[1], q[2], q[3]), r_rq, o, 0, kAuxNT);
          if (has_add) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const uint32_t rb = (resid_pre[k] >> (8 * e)) & 0xFFu;
              q[e] = TK_ABL(8192) ? clamp_i32(q[e] + (int32_t)rb - add_zp, qmin, qmax) : block_join(q[e], rb, lut, add_zp, qmin, qmax);
            }
            if (!TK_ABL(16384 | 2)) __builtin_amdgcn_raw_buffer_store_b32(pack4u(q[0], q[1], q[2], q[3]), r_add, o, 0, kAuxNT);
          }
          if (has_clip) {
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = block_clip(q[e], clip_lo, clip_hi);
            if (!TK_ABL(2)) __builtin_amdgcn_raw_buffer_store_b32(pack4u(q[0], q[1], q[2], q[3]), r_clip, o, 0, kAuxNT);
          }
          if constexpr (ROWU) {
            *reinterpret_cast<v4i*>(tileI + slot[0]) = v4i{q[0], q[1], q[2], q[3]};
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) tileI[slot[e]] = q[e];
          }
        }
      };
      // Lean form for planes of >= 16 pixels, hw % 4 == 0 (the 14x14 256-column tiles, 8x8): the
      // group -> (image, row, column) walk advances incrementally (256 groups = 1024 elements per
      // step: dr rows + dp columns, at most one image wrap since an image run holds >= 256
      // groups), one b128 LDS read of the 4 values and one row of constants per group, the
      // residual join / clip decided at compile time.  The epilogue is VALU-issue-bound at the 1-2
      // waves per SIMD of these launches (profiles/r02m_flat_epilogue_ablations.txt).
      // XR (hw % 4 != 0, the 7x7 stage): a group may cross into the next row; its elements then
      // take that row's constants (per-element selects) and four b32 tile reads.
      auto lean = [&](auto fast_c, auto add_c, auto clip_c, auto xr_c) __attribute__((always_inline)) {
        constexpr bool FAST = decltype(fast_c)::value, ADD = decltype(add_c)::value, CLIP = decltype(clip_c)::value;
        constexpr bool XR = decltype(xr_c)::value;
        const int runG = 16 * hw;             // 4-element groups per image run (BM = 64 rows)
        const int dr = 1024 / hw, dp = 1024 - dr * hw;
        // walk state of a group; its LDS slot is read unconditionally (in bounds of the epilogue
        // area for every lane), lanes past a run store out of range and write back to the sink
        int fg = tid, kk = 0;                  // group within the image run (tid < 256 <= runG)
        int r0 = (int)(((uint64_t)(4 * fg) * mg) >> 40);
        int p0 = 4 * fg - r0 * hw;
        auto slot_of = [&]() __attribute__((always_inline)) { return r0 * kStr + kk * hw + p0; };
        // element e of a group starting at column p0 lies in the next row when p0 + e >= hw
        auto load = [&](int sl, int r, int p, v4u& v, EpiRow& ra, EpiRow& rb) __attribute__((always_inline)) {
          if constexpr (XR) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (uint32_t)tileI[sl + e + (p + e >= hw ? kStr - hw : 0)];
            ra = rowc[r];
            rb = rowc[min(r + 1, BM - 1)];
          } else {
            v = *reinterpret_cast<const v4u*>(tileI + sl);
            ra = rowc[r];
          }
        };
        // software pipeline by one group: group k+1's tile values and row constants are read
        // from LDS before group k's arithmetic and stores
        int sl = slot_of();
        v4u vn;
        EpiRow rn, rn1;
        load(sl, r0, p0, vn, rn, rn1);
#pragma unroll
        for (int k = 0; k < kFlat; ++k) {
          const bool ok = kk < ipt && img0 + kk < nimg && 4 * fg < run;
          const uint32_t o = (uint32_t)(((img0 + kk) * Mrows + m0) * hw + 4 * fg) | (ok ? 0u : kOffDrop);
          int32_t* wslot = ok ? tileI + sl : lut + 512;
          const int pc = p0;                   // this group's first column
          v4u v = vn;
          const EpiRow rr = rn, rr1 = rn1;
          if (k + 1 < kFlat) {
            fg += kGemmThreads;
            r0 += dr;
            p0 += dp;
            if (p0 >= hw) p0 -= hw, ++r0;
            if (fg >= runG) fg -= runG, ++kk, r0 -= BM;
            sl = slot_of();
            load(sl, r0, p0, vn, rn, rn1);
          }
          // per-element row constants (XR: elements past the row end take the next row's)
          uint32_t fold[4], zp[4];
          int32_t bias[4], m[4], sh[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool nx = XR && pc + e >= hw;
            fold[e] = nx ? rr1.fold : rr.fold;
            bias[e] = nx ? rr1.bias : rr.bias;
            zp[e] = nx ? (uint32_t)rr1.zp : (uint32_t)rr.zp;
            m[e] = nx ? rr1.m : rr.m;
            sh[e] = nx ? rr1.s : rr.s;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += fold[e];
          if (!TK_ABL(2)) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i, v), r_conv, o * 4u, 0, kAuxNT);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += (uint32_t)bias[e];
          if (!TK_ABL(2)) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i, v), r_bias, o * 4u, 0, kAuxNT);
          int32_t q[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) q[e] = block_rq<FAST>(v[e], zp[e], m[e], sh[e], mode, zpo, qmin, qmax);
          if (!TK_ABL(2)) __builtin_amdgcn_raw_buffer_store_b32(pack4u(q[0], q[1], q[2], q[3]), r_rq, o, 0, kAuxNT);
          if constexpr (ADD) {
            const uint32_t res = resid_pre[k];
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = block_join(q[e], (res >> (8 * e)) & 0xFFu, lut, add_zp, qmin, qmax);
            if (!TK_ABL(2)) __builtin_amdgcn_raw_buffer_store_b32(pack4u(q[0], q[1], q[2], q[3]), r_add, o, 0, kAuxNT);
          }
          if constexpr (CLIP) {
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = block_clip(q[e], clip_lo, clip_hi);
            if (!TK_ABL(2)) __builtin_amdgcn_raw_buffer_store_b32(pack4u(q[0], q[1], q[2], q[3]), r_clip, o, 0, kAuxNT);
          }
          if constexpr (XR) {
#pragma unroll
            for (int e = 0; e < 4; ++e) wslot[e + (ok && pc + e >= hw ? kStr - hw : 0)] = q[e];
          } else {
            *reinterpret_cast<v4i*>(wslot) = v4i{q[0], q[1], q[2], q[3]};
          }
        }
      };
      auto lean_fast = [&](auto fast_c, auto xr_c) __attribute__((always_inline)) {
        using T = std::true_type;
        using F = std::false_type;
        if (has_add) {
          if (has_clip) lean(fast_c, T{}, T{}, xr_c);
          else lean(fast_c, T{}, F{}, xr_c);
        } else {
          if (has_clip) lean(fast_c, F{}, T{}, xr_c);
          else lean(fast_c, F{}, F{}, xr_c);
        }
      };
      const bool fastrq = s_fast && block_rq_fast_mode(mode);
      if (TK_ABL(65536)) {
      } else if (hw % 4 == 0 && hw >= 16 && !TK_ABL(32768)) {
        if (fastrq) lean_fast(std::true_type{}, std::false_type{});
        else lean_fast(std::false_type{}, std::false_type{});
      } else if (hw >= 16 && !TK_ABL(32768 | 131072)) {
        if (fastrq) lean_fast(std::true_type{}, std::true_type{});
        else lean_fast(std::false_type{}, std::true_type{});
      } else if (hw % 4 == 0 && !TK_ABL(32768)) {
        if (fastrq) groups(std::true_type{}, std::true_type{});
        else groups(std::false_type{}, std::true_type{});
      } else {
        if (fastrq) groups(std::true_type{}, std::false_type{});
        else groups(std::false_type{}, std::false_type{});
      }
    } else if (g.fast_epi && simple_fold && s_fast && !(g.ablate & 0x7D)) {
      // ---- fast path (tile-uniform): 4 consecutive columns x rows (tid>>5) + 8k, every
      // record through a buffer descriptor (masked lanes get an out-of-range offset),
      // requantize in the mul_hi form (block_rq<true>)
      done = true;
      const int c4 = (tid % kLPR) * 4;
      const int col = n0 + c4;
      const bool colok = col < g.N;
      const int img = col / hw;
      const uint32_t cbase = (uint32_t)img * (uint32_t)g.M * (uint32_t)hw + (uint32_t)(col - img * hw);
      const uint32_t n4 = g.out_elems * 4u;
      const auto r_conv = rec_rsrc(g.C, n4), r_bias = rec_rsrc(g.bias_out, n4);
      const auto r_rq = rec_rsrc(g.rq_out, g.out_elems);
      const auto r_add = rec_rsrc(g.add_out, g.has_add ? g.out_elems : 0u);
      const auto r_clip = rec_rsrc(g.clip_out, g.has_clip ? g.out_elems : 0u);
      const int32_t qmin = (int32_t)g.rq.qmin, qmax = (int32_t)g.rq.qmax, zpo = g.rq.zp_out;
      // kernel arguments the row loop needs, held in registers: read through `g` after a
      // store, the compiler reloads them (s_load + lgkmcnt(0), which also drains the LDS reads)
      const int32_t add_zp = g.add_zp, clip_lo = g.clip_lo, clip_hi = g.clip_hi;
      const int mode = g.rq.mode;
      const bool want_shadow = g.shadow_out != nullptr;
      uint32_t offs[kRows];
#pragma unroll
      for (int k = 0; k < kRows; ++k) {
        const int row = m0 + tid / kLPR + kRPI * k;
        offs[k] = (colok && row < g.M) ? cbase + (uint32_t)row * (uint32_t)hw : kOffDrop;
      }
      auto rows = [&](auto add_c, auto clip_c, auto aux_c) __attribute__((always_inline)) {
        constexpr bool ADD = decltype(add_c)::value, CLIP = decltype(clip_c)::value;
        constexpr int AUX = decltype(aux_c)::value;
        if constexpr (ADD) {
          if (!TK_ABL(262144 | 2 | 8192 | 16384)) {
            // residual join: every row's conv / bias_add / requantize records first (3 kRows
            // stores), then the joins, whose residual words (issue_resid) land under those stores
            int32_t qs[kRows][4];
#pragma unroll
            for (int k = 0; k < kRows; ++k) {
              const int lr = tid / kLPR + kRPI * k;
              const EpiRow r = rowc[lr];
              const v4i t = *reinterpret_cast<const v4i*>(tileI + lr * kStr + c4);
              const uint32_t o = offs[k];
              v4u v = __builtin_bit_cast(v4u, t) + r.fold;
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i, v), r_conv, o * 4u, 0, AUX);
              v += (uint32_t)r.bias;
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i, v), r_bias, o * 4u, 0, AUX);
#pragma unroll
              for (int e = 0; e < 4; ++e) qs[k][e] = block_rq<true>(v[e], (uint32_t)r.zp, r.m, r.s, mode, zpo, qmin, qmax);
              __builtin_amdgcn_raw_buffer_store_b32(pack4u(qs[k][0], qs[k][1], qs[k][2], qs[k][3]), r_rq, o, 0, AUX);
            }
#pragma unroll
            for (int k = 0; k < kRows; ++k) {
              const int lr = tid / kLPR + kRPI * k;
              const uint32_t o = offs[k];
              int32_t q[4];
#pragma unroll
              for (int e = 0; e < 4; ++e)
                q[e] = block_join(qs[k][e], (resid_pre[k] >> (8 * e)) & 0xFFu, lut, add_zp, qmin, qmax);
              __builtin_amdgcn_raw_buffer_store_b32(pack4u(q[0], q[1], q[2], q[3]), r_add, o, 0, AUX);
              if constexpr (CLIP) {
#pragma unroll
                for (int e = 0; e < 4; ++e) q[e] = block_clip(q[e], clip_lo, clip_hi);
                __builtin_amdgcn_raw_buffer_store_b32(pack4u(q[0], q[1], q[2], q[3]), r_clip, o, 0, AUX);
              }
              if (want_shadow) *reinterpret_cast<v4i*>(tileI + lr * kStr + c4) = v4i{q[0], q[1], q[2], q[3]};
            }
            return;
          }
        }
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
          const int lr = tid / kLPR + kRPI * k;
          const EpiRow r = rowc[lr];
          int32_t* slot = tileI + lr * kStr + c4;
          const v4i t = *reinterpret_cast<const v4i*>(slot);
          const uint32_t o = offs[k];
          if (TK_ABL(262144)) {
            // profiling: every record stored with no epilogue arithmetic (store side alone)
            const uint32_t b8 = pack4u(t.x, t.y, t.z, t.w);
            __builtin_amdgcn_raw_buffer_store_b128(t, r_conv, o * 4u, 0, AUX);
            __builtin_amdgcn_raw_buffer_store_b128(t, r_bias, o * 4u, 0, AUX);
            __builtin_amdgcn_raw_buffer_store_b32(b8, r_rq, o, 0, AUX);
            if constexpr (ADD) __builtin_amdgcn_raw_buffer_store_b32(b8 ^ resid_pre[k], r_add, o, 0, AUX);
            if constexpr (CLIP) __builtin_amdgcn_raw_buffer_store_b32(b8, r_clip, o, 0, AUX);
            continue;
          }
          // int32 wrap-around arithmetic in unsigned lanes (the reference accumulates mod 2^32)
          v4u v = __builtin_bit_cast(v4u, t) + r.fold;
          if (!TK_ABL(2)) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i, v), r_conv, o * 4u, 0, AUX);
          v += (uint32_t)r.bias;
          if (!TK_ABL(2)) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i, v), r_bias, o * 4u, 0, AUX);
          int32_t q[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) q[e] = block_rq<true>(v[e], (uint32_t)r.zp, r.m, r.s, mode, zpo, qmin, qmax);
          if (!TK_ABL(2)) __builtin_amdgcn_raw_buffer_store_b32(pack4u(q[0], q[1], q[2], q[3]), r_rq, o, 0, AUX);
          if constexpr (ADD) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const uint32_t rb = (resid_pre[k] >> (8 * e)) & 0xFFu;
              q[e] = TK_ABL(8192) ? clamp_i32(q[e] + (int32_t)rb - add_zp, qmin, qmax) : block_join(q[e], rb, lut, add_zp, qmin, qmax);
            }
            if (!TK_ABL(16384 | 2)) __builtin_amdgcn_raw_buffer_store_b32(pack4u(q[0], q[1], q[2], q[3]), r_add, o, 0, AUX);
          }
          if constexpr (CLIP) {
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = block_clip(q[e], clip_lo, clip_hi);
            if (!TK_ABL(2)) __builtin_amdgcn_raw_buffer_store_b32(pack4u(q[0], q[1], q[2], q[3]), r_clip, o, 0, AUX);
          }
          if (want_shadow) *reinterpret_cast<v4i*>(slot) = v4i{q[0], q[1], q[2], q[3]};
        }
      };
      using T = std::true_type;
      using F = std::false_type;
      // always_inline: the epilogue lambdas must not become calls, which would take the address
      // of g and copy every kernel argument to scratch (a 4x slowdown measured)
      auto dispatch = [&](auto aux_c) __attribute__((always_inline)) {
        if (g.has_add) {
          if (g.has_clip) rows(T{}, T{}, aux_c);
          else rows(T{}, F{}, aux_c);
        } else {
          if (g.has_clip) rows(F{}, T{}, aux_c);
          else rows(F{}, F{}, aux_c);
        }
      };
      if (g.fast_epi == 2) dispatch(std::integral_constant<int, 0>{});
      else dispatch(std::integral_constant<int, kAuxNT>{});
    }
  }
  // zero-point folding of V columns: acc - zB[col]*RA[row] - zA[row]*RB[col] + K*zA[row]*zB[col]
  auto fold = [&](int32_t* v, const EpiRow& r, int col, int V) {
    if (simple_fold) {
      for (int q = 0; q < V; ++q) v[q] = (int32_t)((uint32_t)v[q] + r.fold);
    } else {
      for (int q = 0; q < V; ++q) {
        const int cq = min(col + q, g.N - 1);
        const uint32_t zb = zb_vec ? (uint32_t)g.zB_vec[cq] : (uint32_t)g.zB;
        const uint32_t rb = has_rb ? (uint32_t)g.RB[cq] : 0u;
        v[q] = (int32_t)((uint32_t)v[q] - zb * r.ra - r.za * rb + (uint32_t)g.k_eff * r.za * zb);
      }
    }
  };
  const bool store_on = !(g.ablate & 2);
  if (done) {
  } else if (g.vecw >= 4) {
    // 4 consecutive columns x rows (tid>>5) + 8k (BN = 256: (tid>>6) + 4k); the 4 never straddle
    // an image plane
    const int c4 = (tid % kLPR) * 4;
    const int col = n0 + c4;
    const bool colok = col < g.N;
    int64_t cbase, rstride;
    if (g.out_nchw) {
      const int img = col / hw;
      cbase = (int64_t)img * g.M * hw + (col - img * hw);
      rstride = hw;
    } else {
      cbase = col;
      rstride = g.ldc;
    }
    BlockConsts cc[4] = {};
    if (kBlock && !g.ch_is_row)
      for (int q = 0; q < 4; ++q) cc[q] = block_consts(g.bias, g.rq, min(col + q, g.N - 1));
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const int lr = tid / kLPR + kRPI * k;
      const int row = m0 + lr;
      const EpiRow r = rowc[lr];
      const bool ok = colok && row < g.M;
      const int64_t off = cbase + (int64_t)row * rstride;
      const uint32_t resid = (kBlock && g.has_add) ? resid_pre[k] : 0u;
      int32_t* slot = tileI + lr * kStr + c4;
      const v4i t = *reinterpret_cast<const v4i*>(slot);
      int32_t v[4] = {t.x, t.y, t.z, t.w};
      fold(v, r, col, 4);
      epi_apply<4, kBlock>(g, r, v, off, store_on && ok, col, resid, lut, cc);
      if (kBlock && g.shadow_out) *reinterpret_cast<v4i*>(slot) = v4i{v[0], v[1], v[2], v[3]};
    }
  } else if (BN == 128) {
    // one column x rows (tid>>7) + 2k (planes whose length is not a multiple of 4)
    const int lc = tid & (BN - 1);
    const int col = n0 + lc;
    const bool colok = col < g.N;
    BlockConsts cc1{};
    if (kBlock && !g.ch_is_row) cc1 = block_consts(g.bias, g.rq, min(col, g.N - 1));
    int64_t cbase = col, rstride = g.ldc;
    if (g.out_nchw) {
      const int img = col / hw;
      cbase = (int64_t)img * g.M * hw + (col - img * hw);
      rstride = hw;
    }
#pragma unroll 4
    for (int k = 0; k < BM / 2; ++k) {
      const int lr = (tid >> 7) + 2 * k;
      const int row = m0 + lr;
      const EpiRow r = rowc[lr];
      const bool ok = colok && row < g.M;
      const int64_t off = cbase + (int64_t)row * rstride;
      uint32_t resid = 0;
      if (kBlock && g.has_add && ok) resid = g.add_res[off];
      int32_t* slot = tileI + lr * kStr + lc;
      int32_t v[1] = {*slot};
      fold(v, r, col, 1);
      epi_apply<1, kBlock>(g, r, v, off, store_on && ok, col, resid, lut, &cc1);
      if (kBlock && g.shadow_out) *slot = v[0];
    }
  }
  if (kBlock && g.shadow_out && !(g.ablate & 1)) {
    lds_barrier();
    constexpr int kItems = (BM / 16) * BN;
#pragma unroll
    for (int it0 = 0; it0 < kItems; it0 += kGemmThreads) {
      const int it = it0 + tid;
      const int lc = it & (BN - 1);
      const int grp = it / BN;
      const int col = n0 + lc;
      const int ch0 = m0 + grp * 16;
      if (col < g.N && lc < g.tcols && ch0 < g.shadow_cpad) {
        uint32_t w[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          uint32_t word = 0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int ch = ch0 + d * 4 + q;
            uint32_t b = (uint32_t)tileI[(grp * 16 + d * 4 + q) * kStr + lc] ^ g.shadow_xor;
            if (ch >= g.M) b = 0;  // padded channels of a partial group stay zero
            word |= (b & 0xFFu) << (8 * q);
          }
          w[d] = word;
        }
        *reinterpret_cast<v4i*>(g.shadow_out + ((int64_t)(ch0 >> 4) * g.N + col) * 16) =
            v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
      }
    }
  }
}

// ---------------------------------------------------------------- launch by variant key

namespace {
struct GemmKernel {
  GemmVariant key;
  void (*fn)(GemmArgs);
};
#define TK_GEMM_ENTRY(MT, IM, BLK, MODE, RING, WIDE, BN) \
  {GemmVariant{MT, IM, BLK, MODE, RING, WIDE, BN}, gemm_i8_kernel<MT, IM, BLK, MODE, RING, WIDE, BN>},
const GemmKernel kGemmKernels[] = {TK_GEMM_VARIANTS(TK_GEMM_ENTRY)};
#undef TK_GEMM_ENTRY
}  // namespace

int gemm_launch(const GemmVariant& v, dim3 grid, unsigned lds_pad, const GemmArgs& ga, hipStream_t s) {
  for (const GemmKernel& k : kGemmKernels)
    if (k.key == v) {
      hipLaunchKernelGGL(k.fn, grid, dim3(kGemmThreads), lds_pad, s, ga);
      TK_LAUNCH_CHECK();
      return TK_OK;
    }
  set_error("gemm_i8_kernel: no instantiation with MT " + std::to_string(v.mt) + ", im2col " + std::to_string(v.im2col) +
            ", block " + std::to_string(v.block) + ", mode " + std::to_string(v.mode) + ", ring " +
            std::to_string(v.ring) + ", wide " + std::to_string(v.wide) + ", BN " + std::to_string(v.bn));
  return TK_ERR_INVALID_ARG;
}

// ---------------------------------------------------------------- dense

int64_t dense_workspace_bytes(const tk_tensor* data, const tk_tensor* weight) {
  if (!data || !weight || data->ndim != 2 || weight->ndim != 2) return -1;
  return dense_plan(data->shape[0], weight->shape[0], data->shape[1], false).bytes;
}

static int dense_run(const tk_tensor* data, const tk_tensor* weight, tk_tensor* out, const tk_dense_attrs* a,
                     void* workspace, const BlockIO* blk, hipStream_t s) {
  TK_CHECK_ARG(data && weight && out && a && workspace, "null argument");
  TK_CHECK_ARG(data->ndim == 2 && weight->ndim == 2 && out->ndim == 2, "dense expects 2-D tensors");
  TK_CHECK_ARG(is_int8ish(data) && is_int8ish(weight) && is_int(out, 32), "dtypes: int8/uint8 in, int32 out");
  int M = (int)data->shape[0], K = (int)data->shape[1], Nn = (int)weight->shape[0];
  TK_CHECK_ARG(weight->shape[1] == K && out->shape[0] == M && out->shape[1] == Nn, "shape mismatch");
  const DensePlan d = dense_plan(M, Nn, K, blk != nullptr);
  char* ws = (char*)workspace;
  int8_t* dpad = (int8_t*)(ws + d.pad_a);
  int8_t* wpad = (int8_t*)(ws + d.pad_b);
  int32_t* dsum = (int32_t*)(ws + d.sum_a);
  int32_t* wsum = (int32_t*)(ws + d.sum_b);
  int du = is_uint(data, 8), wu = is_uint(weight, 8);
  TK_CHECK_ARG(!(wu && a->kernel_zero_points), "per-unit zero points with uint8 weights are not supported");
  int rc = dense_pad_rows(data, dpad, dsum, d.mrows, d.k_pad, s);
  if (rc) return rc;
  rc = dense_pad_rows(weight, wpad, wsum, d.nrows, d.k_pad, s);
  if (rc) return rc;
  int32_t za = a->input_zero_point - (du ? 128 : 0);
  int32_t zw = a->kernel_zero_point - (wu ? 128 : 0);
  GemmArgs ga{};
  ga.A = dpad;
  ga.B = wpad;
  ga.C = (int32_t*)ptr(out);
  ga.M = M;
  ga.N = Nn;
  ga.lda = d.k_pad;
  ga.ldb = d.k_pad;
  ga.k_pad = d.k_pad;
  ga.k_eff = K;
  ga.zA = za;              // operand A = data
  ga.zB = zw;              // operand B = weights
  ga.zB_vec = a->kernel_zero_points;
  ga.RA = dsum;
  ga.RB = wsum;
  ga.out_nchw = 0;
  ga.ldc = Nn;
  ga.vecw = Nn % 4 == 0 ? 4 : 1;
  ga.ch_is_row = 0;
  TK_CHECK_ARG(!(blk && blk->attrs->has_add), "residual join is supported on conv blocks only");
  rc = setup_block(ga, blk, out, Nn, 1);
  if (rc) return rc;
  ga.shadow_out = nullptr;
  ga.tcols = 128;
  ga.ntiles = d.ntiles;
  ga.ntiles8 = d.ntiles8;
  ga.mtiles = d.mtiles;
  const dim3 grid((unsigned)((int64_t)d.mtiles * d.ntiles8));
  if (d.splits > 1) {
    ga.ws = (int32_t*)(ws + d.partials);
    ga.splits = d.splits;
    ga.kper = d.kper;
    rc = gemm_launch(d.main, dim3(grid.x, 1, (unsigned)d.splits), 0, ga, s);
    return rc ? rc : gemm_launch(d.reduce, grid, 0, ga, s);
  }
  return gemm_launch(d.main, grid, 0, ga, s);
}

int dense_impl(const tk_tensor* data, const tk_tensor* weight, tk_tensor* out, const tk_dense_attrs* a,
               void* workspace, hipStream_t s) {
  return dense_run(data, weight, out, a, workspace, nullptr, s);
}

int dense_block_impl(const tk_tensor* data, const tk_tensor* weight, const tk_tensor* bias, tk_tensor* const* outs,
                     int n_outs, const tk_block_attrs* attrs, void* workspace, hipStream_t s) {
  TK_CHECK_ARG(outs && n_outs >= 3 && outs[0] && attrs, "block needs outputs and attrs");
  BlockIO b{bias, outs, n_outs, attrs, nullptr};
  return dense_run(data, weight, outs[0], &attrs->dense, workspace, &b, s);
}

}  // namespace tk
