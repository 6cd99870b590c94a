// The tail of a fused block, per element, defined once for every conv / dense kernel:
//   conv/dense -> bias_add -> requantize -> [qnn.add] -> [clip]
// bias_add is an int32 add modulo 2^32 that the kernels do on their own vectors; the other
// three records are the functions below.  They take scalars by value and never the kernel
// argument struct: a lambda or callee that touches it sends every kernel argument to scratch.
// The stand-alone ops (tk_elementwise.hip, tk_qnn_ops.hip) and the chain check's requantize
// (tk_chain.hip) stay on rq_apply, the general form, so the check is independent of this file's
// mul_hi form; the chain check and tk_residual.hip share only the table fill.
#pragma once

#include "tk_common.h"

namespace tk {

// min(max(x, lo), hi) in one v_med3_i32 (the compiler only forms it for constant bounds); needs
// lo <= hi, which setup_block guarantees for the clip bounds (see there) and the dtype ranges are
__device__ __forceinline__ int32_t clamp_i32(int32_t x, int32_t lo, int32_t hi) {
  int32_t r;
  asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(lo), "v"(hi));
  return r;
}

__device__ __forceinline__ uint32_t pack4u(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  // low bytes of a, b, c, d -> one dword (two v_perm_b32 + v_or)
  const uint32_t lo = __builtin_amdgcn_perm(b, a, 0x0c0c0400u);
  const uint32_t hi = __builtin_amdgcn_perm(d, c, 0x04000c0cu);
  return lo | hi;
}

// ---------------------------------------------------------------- requantize
// One channel's constants for the kernels that do not stage per-row constants in LDS (direct,
// band, dense tile, the dense GEMM's columns); ch must be a valid channel.
struct BlockConsts {
  int32_t bias, m, s, zp;
};

__device__ __forceinline__ BlockConsts block_consts(const int32_t* bias, const RqParams& rq, int ch) {
  const bool axis = rq.mode >= TK_RQ_AXIS_UPWARD;
  return BlockConsts{bias[ch], axis ? rq.ms[ch] : rq.multiplier, axis ? rq.ss[ch] : rq.shift,
                     rq.zps ? rq.zps[ch] : rq.zp_in};
}

// fixed-point multiply of one element (mode is uniform; the constants may vary per element)
__device__ __forceinline__ int32_t rq_core(int32_t t, int mode, int32_t m, int32_t sh) {
  switch (mode) {
    case TK_RQ_IDENTITY: return t;
    case TK_RQ_TENSOR_POW2: return qms_pow2(t, sh);
    case TK_RQ_TENSOR_TONEAREST:
    case TK_RQ_AXIS_TONEAREST: return qms_tonearest(t, m, sh);
    default: return qms_upward(t, m, sh);
  }
}

// When block_rq<true> is legal: an UPWARD mode and a right shift of at least 2.  The two halves
// are named because they are known at different places: the mode is uniform (the host's fast_epi
// decision rests on it alone, per-axis shifts living on the device), the shift belongs to a row
// (the kernels clear a tile-wide flag, s_fast, on the first row that fails).
__host__ __device__ constexpr bool block_rq_fast_mode(int mode) {
  return mode == TK_RQ_AXIS_UPWARD || mode == TK_RQ_TENSOR_UPWARD;
}
__host__ __device__ constexpr bool block_rq_fast_shift(int32_t s) { return s <= -2; }
__host__ __device__ constexpr bool block_rq_fast_ok(int mode, int32_t s) {
  return block_rq_fast_mode(mode) && block_rq_fast_shift(s);
}

// The requantize record of one bias_add value v (RequantizeLowerInt + clip/cast,
// src/relay/qnn/op/requantize.cc:195-273): clamp(zp_out + FPM(v - zp)), block outputs being 8-bit
// (setup_block), so the clamp is an int32 one.
// FAST (block_rq_fast_ok): with a right shift rs >= 2 the rounding constant 2^(30+rs) of
// qms_upward has a zero low word, so (x·m + 2^(30+rs)) >> (31+rs) only needs the high word of
// x·m (v_mul_hi_i32): (hi + 2^(rs-2)) >> (rs-1).
template <bool FAST>
__device__ __forceinline__ int32_t block_rq(uint32_t v, uint32_t zp, int32_t m, int32_t s, int mode, int32_t zpo,
                                            int32_t qmin, int32_t qmax) {
  const int32_t t = (int32_t)(v - zp);
  int32_t y;
  if constexpr (FAST) {
    const int sh2 = -s - 1;
    y = (int32_t)((uint32_t)__mulhi(t, m) + (1u << (sh2 - 1))) >> sh2;
  } else {
    y = rq_core(t, mode, m, s);
  }
  return clamp_i32((int32_t)((uint32_t)zpo + (uint32_t)y), qmin, qmax);
}

// ---------------------------------------------------------------- residual join
// qnn.add (src/relay/qnn/op/add.cc:40-96): RQ(block) + RQ(residual) - zp_out, clipped to the
// dtype.  With 8-bit operands RQ (RequantizeOrUpcast, op_common.h:186-200: a per-tensor
// requantize to int32, or the value itself) has 256 inputs per side, tabulated once per workgroup:
// thread tid of 256 fills entry tid of both halves of lut[512], the block's side first.
__device__ __forceinline__ int32_t rq_tensor(int32_t t, const RqParams& p) {
  // per-tensor requantize to int32 (every qnn.add operand is validated as per-tensor on the host):
  // rq_apply without the per-channel arrays, which keeps their loads out of the conv kernels
  t = (int32_t)((uint32_t)t - (uint32_t)p.zp_in);
  switch (p.mode) {
    case TK_RQ_TENSOR_POW2: t = qms_pow2(t, p.shift); break;
    case TK_RQ_TENSOR_UPWARD: t = qms_upward(t, p.multiplier, p.shift); break;
    case TK_RQ_TENSOR_TONEAREST: t = qms_tonearest(t, p.multiplier, p.shift); break;
    default: break;
  }
  return (int32_t)((uint32_t)p.zp_out + (uint32_t)t);
}

__device__ __forceinline__ void block_join_lut(int tid, int32_t* lut, bool is_u8, int32_t up_b, int32_t up_r,
                                               const RqParams& pb, const RqParams& pr) {
  const int32_t x = is_u8 ? tid : (int32_t)(int8_t)(uint8_t)tid;  // entry = the value's byte
  lut[tid] = up_b ? x : rq_tensor(x, pb);
  lut[256 + tid] = up_r ? x : rq_tensor(x, pr);
}

// The same table for block_join<true>: the block's side indexed by value - qmin (a lookup is one
// v_lshl_add off a biased base, no byte mask), the residual's by its byte with - zp_out folded in.
__device__ __forceinline__ void block_join_lut_folded(int tid, int32_t* lut, int32_t qmin, int32_t up_b, int32_t up_r,
                                                      const RqParams& pb, const RqParams& pr, int32_t add_zp) {
  const int32_t xb = qmin + tid;
  const int32_t xr = qmin == 0 ? tid : (int32_t)(int8_t)(uint8_t)tid;
  lut[tid] = up_b ? xb : rq_tensor(xb, pb);
  lut[256 + tid] = (int32_t)((uint32_t)(up_r ? xr : rq_tensor(xr, pr)) - (uint32_t)add_zp);
}

// The add record of requantize value q (in [qmin, qmax]) and residual byte rb.
template <bool FOLDED = false>
__device__ __forceinline__ int32_t block_join(int32_t q, uint32_t rb, const int32_t* lut, int32_t add_zp, int32_t qmin,
                                              int32_t qmax) {
  const uint32_t b = FOLDED ? (uint32_t)(lut - qmin)[q] : (uint32_t)lut[q & 0xFF];
  return clamp_i32((int32_t)(b + (uint32_t)lut[256 + rb] - (FOLDED ? 0u : (uint32_t)add_zp)), qmin, qmax);
}

// ---------------------------------------------------------------- clip
// clip of its 8-bit predecessor (python/tvm/topi/math.py:615-640); lo <= hi (setup_block)
__device__ __forceinline__ int32_t block_clip(int32_t q, int32_t lo, int32_t hi) { return clamp_i32(q, lo, hi); }

}  // namespace tk
