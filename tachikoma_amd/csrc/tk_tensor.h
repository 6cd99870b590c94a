// Host-only helpers on tensor descriptors and the error slot.  No HIP: tk_common.h includes this
// for the kernel files, and the plain C++ sources (tk_wire.cc, tk_format.cc, tk_capture_plan.cc)
// include it alone.
#pragma once

#include <stdint.h>

#include <string>

#include "../../include/tachikoma.h"

namespace tk {

// ---------------------------------------------------------------- errors
void set_error(const std::string& msg);
// under the name of the entry point that fails
inline void set_error(const char* who, const std::string& text) { set_error(std::string(who) + ": " + text); }

// ---------------------------------------------------------------- tensors
inline int64_t numel(const tk_tensor* t) {
  int64_t n = 1;
  for (int i = 0; i < t->ndim; ++i) n *= t->shape[i];
  return n;
}
inline int elem_bytes(const tk_tensor* t) { return (t->dtype.bits + 7) / 8; }
inline int64_t nbytes(const tk_tensor* t) { return numel(t) * elem_bytes(t); }
inline char* ptr(const tk_tensor* t) { return static_cast<char*>(t->data) + t->byte_offset; }
inline bool is_int(const tk_tensor* t, int bits) {
  return t->dtype.code == TK_DL_INT && t->dtype.bits == bits && t->dtype.lanes == 1;
}
inline bool is_uint(const tk_tensor* t, int bits) {
  return t->dtype.code == TK_DL_UINT && t->dtype.bits == bits && t->dtype.lanes == 1;
}
inline bool is_int8ish(const tk_tensor* t) { return is_int(t, 8) || is_uint(t, 8); }
inline bool is_integer(const tk_tensor* t) {
  return (t->dtype.code == TK_DL_INT || t->dtype.code == TK_DL_UINT) && t->dtype.lanes == 1 &&
         (t->dtype.bits == 8 || t->dtype.bits == 16 || t->dtype.bits == 32 || t->dtype.bits == 64);
}
inline bool is_f32(const tk_tensor* t) {
  return t->dtype.code == TK_DL_FLOAT && t->dtype.bits == 32 && t->dtype.lanes == 1;
}
inline bool compact(const tk_tensor* t) { return t->strides == nullptr; }

}  // namespace tk
