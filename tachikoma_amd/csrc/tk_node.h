// A module's nodes as the executor (tk_runtime.cc) keeps them and the capture planner
// (tk_capture_plan.cc) reads them.  Host only, no HIP.
#pragma once

#include <vector>

#include "tk_tensor.h"

namespace tk {

// A tensor descriptor owned by the module (shape copied).
struct OwnedTensor {
  tk_tensor t{};
  std::vector<int64_t> shape;
  void assign(const tk_tensor* src) {
    t = *src;
    shape.assign(src->shape, src->shape + src->ndim);
    t.shape = shape.data();
    t.strides = nullptr;
  }
  OwnedTensor() = default;
  OwnedTensor(const OwnedTensor& o) { assign(&o.t); }
  OwnedTensor& operator=(const OwnedTensor& o) {
    assign(&o.t);
    return *this;
  }
};

struct Node {
  tk_node desc{};
  OwnedTensor in[TK_MAX_NODE_INPUTS];
  OwnedTensor out[TK_MAX_NODE_OUTPUTS];
  tk_tensor* outp[TK_MAX_NODE_OUTPUTS] = {};
};

}  // namespace tk
