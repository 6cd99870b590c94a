// The VALU conv kernels for what the MFMA kernels do not take (grouped, depthwise, tiny channel
// counts): the LDS-staged depthwise 3x3 band kernel and the direct kernel, behind conv_direct_run.
// Depthwise 3x3 blocks go to the tile kernel of tk_dw.hip first (conv2d_run, tk_conv.cc).
#include <algorithm>

#include "tk_conv.h"
#include "tk_ops.h"

namespace tk {

// Writes one element of every output of a fused block.  Mirrors, per element:
// nn.bias_add (int32 wrap), RequantizeLowerInt + clip/cast to the out dtype
// (src/relay/qnn/op/requantize.cc:195-273), then clip (python/tvm/topi/math.py:615-640).
template <bool kBlock>
__device__ __forceinline__ void epilogue_store(const GemmArgs& g, int64_t off, int ch, int64_t pix, uint32_t v) {
  g.C[off] = (int32_t)v;
  if (!kBlock) return;
  const BlockConsts c = block_consts(g.bias, g.rq, ch);
  v += (uint32_t)c.bias;
  g.bias_out[off] = (int32_t)v;
  const int32_t q = block_rq<false>(v, (uint32_t)c.zp, c.m, c.s, g.rq.mode, g.rq.zp_out, (int32_t)g.rq.qmin, (int32_t)g.rq.qmax);
  g.rq_out[off] = (uint8_t)q;
  int32_t last = q;
  if (g.has_clip) {
    last = block_clip(q, g.clip_lo, g.clip_hi);
    g.clip_out[off] = (uint8_t)last;
  }
  if (g.shadow_out) {
    g.shadow_out[((int64_t)(ch >> 4) * g.N + pix) * 16 + (ch & 15)] = (uint8_t)((uint32_t)last ^ g.shadow_xor);
    if (ch == g.M - 1)  // the padded channels of the last group are written as 0
      for (int c2 = ch + 1; c2 < g.shadow_cpad; ++c2) g.shadow_out[((int64_t)(c2 >> 4) * g.N + pix) * 16 + (c2 & 15)] = 0;
  }
}

// Direct (VALU) grouped / depthwise / tiny-channel convolution on NCHW int8/uint8.
// out[n][o][oh][ow] = Σ_{c in group(o), r, s} (a - za)(w - zw[o]); padded taps contribute 0.
template <typename Tx, typename Tw, bool kBlock>
__global__ __launch_bounds__(256) void direct_conv_kernel(const Tx* __restrict__ x, const Tw* __restrict__ w,
                                                          int N, int C, int H, int W, int O,
                                                          int OH, int OW, int KH, int KW, int sh, int sw, int pt, int pl,
                                                          int dh, int dw, int groups, int32_t za, int32_t zw,
                                                          const int32_t* __restrict__ zw_vec, GemmArgs g) {
  int64_t total = (int64_t)N * O * OH * OW;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int cg = C / groups, og = O / groups;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += stride) {
    int ow = (int)(i % OW);
    int64_t t = i / OW;
    int oh = (int)(t % OH);
    t /= OH;
    int o = (int)(t % O);
    int n = (int)(t / O);
    int grp = o / og;
    int32_t zwo = zw_vec ? zw_vec[o] : zw;
    uint32_t acc = 0;
    for (int c = 0; c < cg; ++c) {
      int ci = grp * cg + c;
      const Tx* plane = x + ((int64_t)n * C + ci) * H * W;
      const Tw* wk = w + (((int64_t)o * cg + c) * KH) * KW;
      for (int r = 0; r < KH; ++r) {
        int ih = oh * sh - pt + r * dh;
        if (ih < 0 || ih >= H) continue;
        for (int s = 0; s < KW; ++s) {
          int iw = ow * sw - pl + s * dw;
          if (iw < 0 || iw >= W) continue;
          int32_t a = (int32_t)plane[ih * W + iw] - za;
          int32_t b = (int32_t)wk[r * KW + s] - zwo;
          acc += (uint32_t)(a * b);
        }
      }
    }
    int64_t pix = (int64_t)n * OH * OW + (int64_t)oh * OW + ow;
    epilogue_store<kBlock>(g, i, o, pix, acc);
  }
}

// Depthwise 3x3 conv (groups == C == O, the MobileNetV2 layers) with the fused block epilogue.
// One workgroup = one image x 16 channels x a band of BH output rows:
//   * the input band plus halo is staged planar in LDS ([16][rows][cols], bytes, taps outside
//     the image hold the input zero point so they contribute 0, legalizations.py:195-226), the
//     per-channel weights minus their zero point as int32;
//   * lanes run along output columns, V consecutive pixels each, so every record store is a
//     contiguous row segment of an NCHW plane (b128 int32 / b32 int8 when V = 4);
//   * the final 8-bit values are parked in LDS and written to the next conv's channel-blocked
//     shadow as one 16-byte chunk (the 16 channels) per pixel.
// Same arithmetic as direct_conv_kernel / epilogue_store (int32 wrap-around accumulation).
template <typename Tx, typename Tw, int V>
__global__ __launch_bounds__(256) void dw3x3_kernel(const Tx* __restrict__ x, const Tw* __restrict__ w, int C, int H,
                                                    int W, int OH, int OW, int sh, int sw, int pt, int pl, int32_t za,
                                                    int32_t zw, const int32_t* __restrict__ zw_vec, int BH, int bands,
                                                    int Wp, GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dsm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int bid = blockIdx.x;
  const int band = bid % bands;
  bid /= bands;
  const int cgroups = C / 16;
  const int cgrp = bid % cgroups, n = bid / cgroups;
  const int c0 = cgrp * 16;
  const int oh0 = band * BH;
  const int bh = min(BH, OH - oh0);
  const int rows_in = (bh - 1) * sh + 3;
  const int ih0 = oh0 * sh - pt;
  uint8_t* tin = dsm;
  const int tin_bytes = (16 * rows_in * Wp + 15) & ~15;
  int32_t* wts = reinterpret_cast<int32_t*>(dsm + tin_bytes);
  uint8_t* tout = dsm + tin_bytes + 16 * 9 * 4;
  // ---- stage the band: (channel, input row) rows of Wp = W + 8 bytes, input column iw at
  // byte 4 + iw (4-byte aligned interior; the 4-byte halos hold the zero point); one dword
  // per lane (W % 4 == 0, W <= 248), 8 rows per wave at a time so that 8 loads are in flight
  const uint32_t fill4 = 0x01010101u * (uint8_t)za;
  const int nrows = 16 * rows_in;
  const int words = W / 4;
  for (int r0 = wave; r0 < nrows; r0 += 32) {
    uint32_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = r0 + 4 * u;
      const int c = r / rows_in, lr = r - c * rows_in;
      const int ih = ih0 + lr;
      const bool ok = r < nrows && ih >= 0 && ih < H && lane < words;
      const uint32_t* src = reinterpret_cast<const uint32_t*>(
          reinterpret_cast<const uint8_t*>(x) + (((int64_t)n * C + c0 + c) * H + (ok ? ih : 0)) * W);
      v[u] = ok ? src[lane] : fill4;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = r0 + 4 * u;
      if (r < nrows) {
        uint32_t* row = reinterpret_cast<uint32_t*>(tin + r * Wp);
        if (lane < words) row[1 + lane] = v[u];
        else if (lane == words) row[0] = fill4, row[1 + words] = fill4;
      }
    }
  }
  if (tid < 16 * 9) {
    const int c = tid / 9;
    wts[tid] = (int32_t)w[(int64_t)(c0 + c) * 9 + (tid - c * 9)] - (zw_vec ? zw_vec[c0 + c] : zw);
  }
  __syncthreads();
  // ---- 9 taps + epilogue, V pixels of one channel row per item
  const int owv = OW / V;
  const int items = 16 * bh * owv;
  const int qmin = (int)g.rq.qmin, qmax = (int)g.rq.qmax;
  for (int it = tid; it < items; it += 256) {
    const int vv = it % owv;
    const int t = it / owv;
    const int row = t % bh, c = t / bh;
    const int ch = c0 + c;
    int32_t acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const uint8_t* base = tin + (c * rows_in + row * sh + r) * Wp;
#pragma unroll
      for (int s2 = 0; s2 < 3; ++s2) {
        const int32_t wv = wts[c * 9 + r * 3 + s2];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const int32_t a = (int32_t)(Tx)base[(vv * V + e) * sw + s2 + 4 - pl] - za;
          acc[e] = (int32_t)((uint32_t)acc[e] + (uint32_t)(a * wv));
        }
      }
    }
    const int oh = oh0 + row, ow = vv * V;
    const int64_t off = (((int64_t)n * C + ch) * OH + oh) * OW + ow;
    int32_t v[V];
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = acc[e];
    st_i32<V>(g.C + off, v, false);
    const BlockConsts k = block_consts(g.bias, g.rq, ch);
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = (int32_t)((uint32_t)v[e] + (uint32_t)k.bias);
    st_i32<V>(g.bias_out + off, v, false);
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = block_rq<false>((uint32_t)v[e], (uint32_t)k.zp, k.m, k.s, g.rq.mode, g.rq.zp_out, qmin, qmax);
    st_i8<V>(g.rq_out + off, v, false);
    if (g.has_clip) {
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = block_clip(v[e], g.clip_lo, g.clip_hi);
      st_i8<V>(g.clip_out + off, v, false);
    }
#pragma unroll
    for (int e = 0; e < V; ++e) tout[((row * OW) + ow + e) * 16 + c] = (uint8_t)((uint32_t)v[e] ^ g.shadow_xor);
  }
  if (!g.shadow_out) return;
  __syncthreads();
  // ---- shadow: 16 channels of one pixel per 16-byte store, contiguous across lanes
  const int64_t pix0 = ((int64_t)n * OH + oh0) * OW;
  for (int p = tid; p < bh * OW; p += 256)
    *reinterpret_cast<v4i*>(g.shadow_out + ((int64_t)cgrp * g.N + pix0 + p) * 16) =
        *reinterpret_cast<const v4i*>(tout + p * 16);
}

// ---------------------------------------------------------------- host wrapper

// f(Tx{}, Tw{}) with the element types of an 8-bit data / weight pair
template <typename F>
static void with_i8_types(bool data_u8, bool weight_u8, F&& f) {
  if (data_u8 && weight_u8) f(uint8_t{}, uint8_t{});
  else if (data_u8) f(uint8_t{}, int8_t{});
  else if (weight_u8) f(int8_t{}, uint8_t{});
  else f(int8_t{}, int8_t{});
}

int conv_direct_run(const tk_tensor* data, const tk_tensor* weight, const ConvGeom& g, const tk_conv2d_attrs* a,
                    const GemmArgs& ga, bool block, hipStream_t s) {
  const bool du = is_uint(data, 8), wu = is_uint(weight, 8);
  // depthwise 3x3 blocks: the LDS-staged band kernel (see dw3x3_kernel)
  // (large planes only: on 7x7 / 14x14 planes and strided 28x28 ones the generic kernel measured
  // faster, the band staging does not amortise; MobileNetV2 dw layers 1.2-2x faster otherwise)
  const int64_t ohw = (int64_t)g.OH * g.OW;
  if (block && a->groups == g.C && g.C == g.O && g.C % 16 == 0 && g.KH == 3 && g.KW == 3 && a->dilation[0] == 1 &&
      a->dilation[1] == 1 && ((a->strides[0] == 1 && ohw >= 784) || ohw >= 3136) && env_int("TK_DW", 1)) {
    const int sh = a->strides[0], sw = a->strides[1];
    // output pixels per workgroup and channel: whole planes up to 1024 pixels, else bands of
    // ~512 (stride 1) / ~256 (stride 2) pixels (measured on MobileNetV2's 112x112 and 56x56 layers)
    const int budget = env_int("TK_DW_BUDGET", sh == 1 ? 512 : 256);
    const int BH = g.OH * g.OW <= 1024 ? g.OH : std::max(1, budget / g.OW);
    const int bands = (g.OH + BH - 1) / BH;
    const int Wp = g.W + 8;  // input row + 4-byte halos (see dw3x3_kernel)
    const int rows_max = (BH - 1) * sh + 3;
    const size_t lds = (size_t)((16 * rows_max * Wp + 15) & ~15) + 16 * 9 * 4 + (size_t)BH * g.OW * 16;
    const bool fits = g.W % 4 == 0 && g.W <= 248 && a->padding[1] <= 4 && (g.OW - 1) * sw + 2 - a->padding[1] < g.W + 4;
    if (lds <= 64 * 1024 && fits) {
      const unsigned grid = (unsigned)((int64_t)g.N * (g.C / 16) * bands);
      with_i8_types(du, wu, [&](auto tx, auto tw) {
        using TX = decltype(tx);
        using TW = decltype(tw);
        auto launch = [&](auto kern) {
          hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, (const TX*)ptr(data), (const TW*)ptr(weight), g.C, g.H,
                             g.W, g.OH, g.OW, sh, sw, a->padding[0], a->padding[1], a->input_zero_point,
                             a->kernel_zero_point, a->kernel_zero_points, BH, bands, Wp, ga);
        };
        if (g.OW % 4 == 0) launch(dw3x3_kernel<TX, TW, 4>);
        else launch(dw3x3_kernel<TX, TW, 1>);
      });
      TK_LAUNCH_CHECK();
      return TK_OK;
    }
  }
  // grouped / depthwise / tiny channel counts: direct VALU kernel on NCHW
  const int64_t total = (int64_t)g.N * g.O * g.OH * g.OW;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 8192));
  with_i8_types(du, wu, [&](auto tx, auto tw) {
    using TX = decltype(tx);
    using TW = decltype(tw);
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, (const TX*)ptr(data), (const TW*)ptr(weight), g.N, g.C, g.H,
                         g.W, g.O, g.OH, g.OW, g.KH, g.KW, a->strides[0], a->strides[1], a->padding[0], a->padding[1],
                         a->dilation[0], a->dilation[1], a->groups, a->input_zero_point, a->kernel_zero_point,
                         a->kernel_zero_points, ga);
    };
    if (block) launch(direct_conv_kernel<TX, TW, true>);
    else launch(direct_conv_kernel<TX, TW, false>);
  });
  TK_LAUNCH_CHECK();
  return TK_OK;
}

}  // namespace tk
