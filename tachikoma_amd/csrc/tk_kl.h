// The kl_divergence threshold search on the device (tk_kl.hip): the constants of the error bound
// that the evaluate kernel carries beside each divergence, and the geometry.
#pragma once

#include "tk_common.h"

namespace tk {

constexpr int kKlMaxBins = 8192;  // counts of one record held in LDS as int32 (num_bins is odd: <= 8191)
constexpr int kKlLanes = 256;     // candidates per workgroup of the evaluate kernel: four waves share the counts
constexpr float kKlEps = 0.0001f; // smooth()'s eps (tk_calibrate.cc)

constexpr double kKlU = 0x1p-24;          // unit roundoff of float32
constexpr double kKlHostLogUlps = 2.0;    // assumed bound on the host logf's error, in ulps (glibc documents < 1)
// |fl32(p * logf(r)) - p * log(r) as the device has it| <= kKlTermRel * |device term| + kKlTermAbs:
// 2 ulp of the log are <= 4u relative, the float32 product adds u, and the last u covers the cross
// terms and the device's float64 log and product (a few 2^-53); kKlTermAbs is the product's underflow.
constexpr double kKlTermRel = (2.0 * kKlHostLogUlps + 2.0) * kKlU;
constexpr double kKlTermAbs = 0x1p-149;
// each float32 add of the host's running sum rounds by <= u |exact sum|; 2^-51 |D| covers the float64 add
// of the device's running sum and the use of |D| for the exact sum's size
constexpr double kKlAddRel = kKlU + 0x1p-51;
constexpr double kKlBoundSlack = 1.0 + 0x1p-30;  // the bound itself is evaluated in rounded float64

}  // namespace tk
