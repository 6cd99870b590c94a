// The functions the kernel files (.hip) define for the executor (tk_runtime.cc) and the packed
// capture (tk_capture.cc), declared once.  The files that define them include this too.
#pragma once

#include "tk_capture_plan.h"
#include "tk_common.h"
#include "tk_wire.h"

namespace tk {

// tk_elementwise.hip
int requantize_impl(const tk_tensor* x, tk_tensor* y, const tk_requantize_attrs* a, hipStream_t s);
int bias_add_impl(const tk_tensor* x, const tk_tensor* b, tk_tensor* y, int axis, hipStream_t s);
int clip_impl(const tk_tensor* x, tk_tensor* y, int64_t lo, int64_t hi, hipStream_t s);
int cast_impl(const tk_tensor* x, tk_tensor* y, hipStream_t s);
int qnn_add_impl(const tk_tensor* a, const tk_tensor* b, tk_tensor* y, const tk_qnn_add_attrs* at, hipStream_t s);
int max_pool_impl(const tk_tensor* x, tk_tensor* y, const tk_pool2d_attrs* a, hipStream_t s);
int max_pool_shadow_impl(const tk_tensor* x, const void* x_shadow, tk_tensor* y, const tk_pool2d_attrs* a,
                         void* y_shadow, hipStream_t s);
int avg_pool_impl(const tk_tensor* x, tk_tensor* y, const tk_pool2d_attrs* a, hipStream_t s);
int global_avg_pool_impl(const tk_tensor* x, tk_tensor* y, hipStream_t s);
int copy_impl(const tk_tensor* x, tk_tensor* y, hipStream_t s);
int pad_impl(const tk_tensor* x, tk_tensor* y, const tk_pad_attrs* a, hipStream_t s);
int postops_impl(const tk_tensor* acc, const tk_tensor* sum_src, tk_tensor* y, const tk_postops_attrs* a,
                 hipStream_t s);
// tk_residual.hip
int add_block_impl(const tk_tensor* a, const tk_tensor* b, tk_tensor* const* outs, int n_outs,
                   const tk_add_block_attrs* at, void* shadow, hipStream_t s);
// tk_trace.hip: what the executor's copy kernels and the packed capture launch
int host_copy_impl(const void* const* src, void* const* dst, const int64_t* bytes, int n, hipStream_t s);
int pack_records_impl(const PackRec* table, int nrec, int64_t blocks, void* mirror, hipStream_t s);
int wire_encode_impl(const WireSegDev* segs, int64_t n_seg, uint32_t* cursor, void* wire, int64_t wire_bytes,
                     hipStream_t s);
// tk_realize.hip (the float ops; the last four are tk_elementwise.hip's float paths)
int ewise_impl(const tk_tensor* x, const tk_tensor* r, tk_tensor* y, const tk_ewise_attrs* a, hipStream_t s);
int conv2d_f32_impl(const tk_tensor* x, const tk_tensor* w, tk_tensor* y, const tk_conv2d_attrs* a, hipStream_t s);
int dense_f32_impl(const tk_tensor* x, const tk_tensor* w, tk_tensor* y, hipStream_t s);
int cast_f32_impl(const tk_tensor* x, tk_tensor* y, hipStream_t s);
int bias_add_f32_impl(const tk_tensor* x, const tk_tensor* b, tk_tensor* y, int axis, hipStream_t s);
int global_avg_pool_f32_impl(const tk_tensor* x, tk_tensor* y, hipStream_t s);
int max_pool_f32_impl(const tk_tensor* x, tk_tensor* y, const tk_pool2d_attrs* a, hipStream_t s);
// tk_conv_prep.hip (packed weight, shadow), tk_conv.cc (conv), tk_gemm.hip (dense)
int64_t conv_packed_weight_bytes(const tk_tensor* weight, int groups);
int conv_pack_weight(const tk_tensor* weight, int groups, void* packed, int32_t* sums, hipStream_t s);
int64_t conv_shadow_bytes(const tk_tensor* data);
int64_t conv_scratch_bytes(const tk_tensor* data, const tk_tensor* weight, const tk_conv2d_attrs* a, int block);
int make_shadow_impl(const tk_tensor* data, void* shadow, hipStream_t s);
int conv2d_prepared_impl(const tk_tensor* data, const void* shadow, const tk_tensor* weight, const void* packed,
                         const int32_t* sums, tk_tensor* out, const tk_conv2d_attrs* a, void* scratch, hipStream_t s);
int64_t conv2d_workspace_bytes(const tk_tensor* data, const tk_tensor* weight, const tk_conv2d_attrs* a);
int conv2d_impl(const tk_tensor* data, const tk_tensor* weight, tk_tensor* out, const tk_conv2d_attrs* a,
                void* workspace, hipStream_t s);
int64_t dense_workspace_bytes(const tk_tensor* data, const tk_tensor* weight);
int dense_impl(const tk_tensor* data, const tk_tensor* weight, tk_tensor* out, const tk_dense_attrs* a,
               void* workspace, hipStream_t s);
int conv2d_block_impl(const tk_tensor* data, const void* shadow, const tk_tensor* weight, const void* packed,
                      const int32_t* sums, const tk_tensor* bias, tk_tensor* const* outs, int n_outs,
                      const tk_block_attrs* attrs, void* scratch, void* shadow_out, hipStream_t s);
int dense_block_impl(const tk_tensor* data, const tk_tensor* weight, const tk_tensor* bias, tk_tensor* const* outs,
                     int n_outs, const tk_block_attrs* attrs, void* workspace, hipStream_t s);
int conv2d_block_algos_impl(const tk_tensor* data, const tk_tensor* weight, const tk_block_attrs* attrs,
                            int32_t* algos, int max_algos);
int conv2d_block_algo_info_impl(const tk_tensor* data, const tk_tensor* weight, const tk_block_attrs* attrs, int algo,
                                char* buf, int len);
// tk_qnn_ops.hip
int qnn_quantize_impl(const tk_tensor* x, tk_tensor* y, const tk_qparams_attrs* a, hipStream_t s);
int qnn_dequantize_impl(const tk_tensor* x, tk_tensor* y, const tk_qparams_attrs* a, hipStream_t s);
int qnn_binary_impl(const tk_tensor* a, const tk_tensor* b, tk_tensor* y, const tk_qnn_binary_attrs* at,
                    hipStream_t s);
int qnn_concatenate_impl(const tk_tensor* const* xs, int n_in, tk_tensor* y, const tk_concat_attrs* a,
                         hipStream_t s);
int transpose_impl(const tk_tensor* x, tk_tensor* y, const tk_transpose_attrs* a, hipStream_t s);
int qnn_leaky_relu_impl(const tk_tensor* x, tk_tensor* y, const tk_leaky_relu_attrs* a, hipStream_t s);
int qnn_simulated_impl(bool quant, const tk_tensor* x, tk_tensor* y, const tk_simq_attrs* a, hipStream_t s);
int requantize_fp_impl(const tk_tensor* x, tk_tensor* y, const tk_requantize_fp_attrs* a, hipStream_t s);
int qnn_binary_fp_impl(const tk_tensor* a, const tk_tensor* b, tk_tensor* y, const tk_qnn_binary_fp_attrs* at,
                       hipStream_t s);
int qnn_lookup_impl(const tk_tensor* x, tk_tensor* y, const void* table, hipStream_t s);
int qnn_conv2d_transpose_impl(const tk_tensor* x, const tk_tensor* w, tk_tensor* y, const tk_conv2d_transpose_attrs* a,
                              hipStream_t s);

}  // namespace tk
