// Operand preparation of the MFMA conv / dense kernels (tk_gemm.hip): the packed weight with its
// row sums, the channel-blocked shadow of an NCHW tensor, the padded rows of a dense operand and
// the per-pixel patch sums a non-zero kernel zero point needs.
#include <algorithm>

#include "tk_conv.h"
#include "tk_ops.h"

namespace tk {

// ---------------------------------------------------------------- operand preparation

// pack OIHW (int8/uint8) -> [Cout_rows][k_pad], k = (kh*KW + kw)*cin_pad + c ; row sums over real taps.
// groups == 1 only (grouped convs take the direct kernel).
__global__ __launch_bounds__(256) void pack_weight_kernel(const int8_t* __restrict__ w, int8_t* __restrict__ packed,
                                                          int32_t* __restrict__ sums, int Cout, int Cin, int KH, int KW,
                                                          int cin_pad, int k_pad, int xor_u8) {
  int o = blockIdx.x;
  int8_t* dst = packed + (int64_t)o * k_pad;
  int32_t s = 0;
  for (int k = threadIdx.x; k < k_pad; k += blockDim.x) {
    int tap = k / cin_pad;
    int c = k - tap * cin_pad;
    int8_t v = 0;
    if (o < Cout && tap < KH * KW && c < Cin) {
      int kh = tap / KW, kw = tap - (tap / KW) * KW;
      uint8_t raw = (uint8_t)w[(((int64_t)o * Cin + c) * KH + kh) * KW + kw];
      v = (int8_t)(xor_u8 ? (raw ^ 0x80) : raw);
      s += v;
    }
    dst[k] = v;
  }
  __shared__ int32_t red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0 && o < Cout) sums[o] = red[0];
}

// NCHW int8/uint8 -> shadow [cin_pad/16][N*HW][16]; padded channels 0; uint8 xor 0x80.
// One thread per (16-channel chunk, pixel); lanes run along pixels, so each channel
// plane read is a contiguous 64-byte span and the 16-byte stores are contiguous.
__global__ __launch_bounds__(256) void shadow_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ y, int N,
                                                     int C, int HW, int cin_pad, int xor_u8) {
  int chunks = cin_pad / 16;
  int64_t total = (int64_t)N * HW * chunks;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += stride) {
    int64_t q = t / HW;          // (n, chunk)
    int pix = (int)(t - q * HW);
    int chunk = (int)(q % chunks);
    int n = (int)(q / chunks);
    uint8_t v[16];
    const uint8_t* src = x + ((int64_t)n * C) * HW + pix;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      int c = chunk * 16 + j;
      uint8_t b = 0;
      if (c < C) b = xor_u8 ? (uint8_t)(src[(int64_t)c * HW] ^ 0x80) : src[(int64_t)c * HW];
      v[j] = b;
    }
    __builtin_memcpy(y + ((int64_t)chunk * N * HW + (int64_t)n * HW + pix) * 16, v, 16);
  }
}

// dense data [M][K] -> [M_rows][k_pad] (zero padded, uint8 xor 0x80) + row sums.
__global__ __launch_bounds__(256) void pad_rows_kernel(const uint8_t* __restrict__ x, int8_t* __restrict__ y,
                                                       int32_t* __restrict__ sums, int M, int K, int k_pad, int xor_u8) {
  int m = blockIdx.x;
  int32_t s = 0;
  for (int k = threadIdx.x; k < k_pad; k += blockDim.x) {
    int8_t v = 0;
    if (m < M && k < K) {
      uint8_t raw = x[(int64_t)m * K + k];
      v = (int8_t)(xor_u8 ? (raw ^ 0x80) : raw);
      s += v;
    }
    y[(int64_t)m * k_pad + k] = v;
  }
  __shared__ int32_t red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0 && m < M && sums) sums[m] = red[0];
}

// Σ over the real taps/channels of the (zero-point-filled) patch of every output pixel:
// only needed when the kernel zero point is non-zero.
__global__ __launch_bounds__(256) void patch_sum_kernel(const int8_t* __restrict__ shadow, int32_t* __restrict__ out,
                                                        GemmArgs g, int Cin) {
  int64_t total = g.N;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int8_t zpa = (int8_t)(g.fill & 0xFF);
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < total; p += stride) {
    int hw = g.OH * g.OW;
    int img = (int)(p / hw);
    int rem = (int)(p - (int64_t)img * hw);
    int oh = rem / g.OW, ow = rem - (rem / g.OW) * g.OW;
    int32_t s = 0;
    for (int kh = 0; kh < g.KH; ++kh) {
      int ih = oh * g.sh - g.pt + kh * g.dh;
      for (int kw = 0; kw < g.KW; ++kw) {
        int iw = ow * g.sw - g.pl + kw * g.dw;
        if (ih < 0 || ih >= g.H || iw < 0 || iw >= g.W) {
          s += (int32_t)zpa * Cin;
        } else {
          const int64_t pix = ((int64_t)img * g.H + ih) * g.W + iw;
          for (int c = 0; c < Cin; ++c) s += shadow[((int64_t)(c >> 4) * g.in_pix + pix) * 16 + (c & 15)];
        }
      }
    }
    out[p] = s;
  }
}

// ---------------------------------------------------------------- host wrappers

int64_t conv_packed_weight_bytes(const tk_tensor* weight, int groups) {
  if (!weight || weight->ndim != 4 || groups != 1) return 0;
  int O = (int)weight->shape[0], C = (int)weight->shape[1], KH = (int)weight->shape[2], KW = (int)weight->shape[3];
  int cin_pad = (C + 15) / 16 * 16;
  int64_t k_pad = ((int64_t)KH * KW * cin_pad + kBK - 1) / kBK * kBK;
  int64_t rows = (O + 127) / 128 * 128;
  // + the chunked image of a KHxKW > 1 weight for the image-tile kernel (tk_conv_img.hip)
  return rows * k_pad + conv_img_chunked_bytes((int)rows, cin_pad, KH * KW);
}

int conv_pack_weight(const tk_tensor* weight, int groups, void* packed, int32_t* sums, hipStream_t s) {
  TK_CHECK_ARG(weight && packed && sums && weight->ndim == 4 && groups == 1, "bad arguments");
  TK_CHECK_ARG(is_int8ish(weight), "weight must be int8/uint8");
  int O = (int)weight->shape[0], C = (int)weight->shape[1], KH = (int)weight->shape[2], KW = (int)weight->shape[3];
  int cin_pad = (C + 15) / 16 * 16;
  int k_pad = (KH * KW * cin_pad + kBK - 1) / kBK * kBK;
  int rows = (O + 127) / 128 * 128;
  hipLaunchKernelGGL(pack_weight_kernel, dim3(rows), dim3(256), 0, s, (const int8_t*)ptr(weight), (int8_t*)packed, sums,
                     O, C, KH, KW, cin_pad, k_pad, (int)is_uint(weight, 8));
  TK_LAUNCH_CHECK();
  return conv_img_pack(weight, (int8_t*)packed + (int64_t)rows * k_pad, rows, cin_pad, s);
}

int64_t conv_shadow_bytes(const tk_tensor* data) {
  if (!data || data->ndim != 4) return 0;
  int64_t cin_pad = (data->shape[1] + 15) / 16 * 16;
  return data->shape[0] * data->shape[2] * data->shape[3] * cin_pad;
}

int make_shadow_impl(const tk_tensor* data, void* shadow, hipStream_t s) {
  TK_CHECK_ARG(data && shadow && data->ndim == 4 && is_int8ish(data), "data must be 4-D int8/uint8");
  int N = (int)data->shape[0], C = (int)data->shape[1], HW = (int)(data->shape[2] * data->shape[3]);
  int cin_pad = (C + 15) / 16 * 16;
  int64_t total = (int64_t)N * HW * (cin_pad / 16);
  int grid = (int)std::min<int64_t>((total + 255) / 256, 2048);
  hipLaunchKernelGGL(shadow_kernel, dim3(std::max(grid, 1)), dim3(256), 0, s, (const uint8_t*)ptr(data),
                     (uint8_t*)shadow, N, C, HW, cin_pad, (int)is_uint(data, 8));
  TK_LAUNCH_CHECK();
  return TK_OK;
}

int conv_patch_sums(const void* shadow, int32_t* out, const GemmArgs& ga, int cin, hipStream_t s) {
  int grid = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)ga.N + 255) / 256, 4096));
  hipLaunchKernelGGL(patch_sum_kernel, dim3(grid), dim3(256), 0, s, (const int8_t*)shadow, out, ga, cin);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

int dense_pad_rows(const tk_tensor* x, int8_t* padded, int32_t* sums, int rows_pad, int k_pad, hipStream_t s) {
  hipLaunchKernelGGL(pad_rows_kernel, dim3(rows_pad), dim3(256), 0, s, (const uint8_t*)ptr(x), padded, sums,
                     (int)x->shape[0], (int)x->shape[1], k_pad, (int)is_uint(x, 8));
  TK_LAUNCH_CHECK();
  return TK_OK;
}

}  // namespace tk
