// Trace wire format: int32 trace records leave the device losslessly narrowed and are widened
// on the host (tk_wire.cc: host decoder, thread pool and reference encoder; tk_elementwise.hip:
// the device encoder; tk_runtime.cc: the packed capture that uses them).
//
// A record of n int32 elements is cut into blocks of kWireBlock elements and segments of
// kWireSegBlocks blocks (the last block / segment of a record may be short).  The coded value of
// an element is the element itself or, for a differenced record, element - predecessor element
// with int32 wrap-around.  A block is coded as base (the minimum coded value) plus unsigned
// offsets of `width` bytes each, width 0..4 from the block's range in unsigned 32-bit arithmetic
// (0: constant block, 4: raw escape).
//
// Wire buffer:  u32 start[n_seg]  (padded to 64 B)  |  payload
//   start[i] * 64 is the payload offset of segment i; the device takes it from one cursor per
//   buffer, so segments lie densely in completion order.
// Segment of nb blocks:
//   i32 base[nb] (padded to 16 B) | u8 width[nb] (padded to 16 B) | block payloads | pad to 64 B
// Block payload of cnt elements: `width` byte planes of cnt bytes, plane k holding byte k of every
// offset (a full block's planes are 256 B, so the device writes them with 16-byte stores and the
// host widens them with byte-to-dword vector loops).
#pragma once

#include <stdint.h>

#include <vector>

namespace tk {

constexpr int kWireBlock = 256;
constexpr int kWireSegBlocks = 64;
constexpr int kWireSegElems = kWireBlock * kWireSegBlocks;

inline int64_t wire_align(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
inline int64_t wire_table_bytes(int64_t n_seg) { return wire_align(4 * n_seg, 64); }
inline int64_t wire_header_bytes(int nb) { return wire_align(4 * (int64_t)nb, 16) + wire_align(nb, 16); }
// worst case (every block raw) of a segment of n elements
inline int64_t wire_seg_bound(int n) {
  return wire_align(wire_header_bytes((n + kWireBlock - 1) / kWireBlock) + 4 * (int64_t)n, 64);
}

// device encoder's view of a segment
struct WireSegDev {
  const int32_t* src;
  const int32_t* prev;  // differenced against (device), or null
  int32_t n;
  int32_t pad;
};
// host decoder's view: destinations in the trace image, any alignment
struct WireSegHost {
  char* dst;
  const char* prev;  // differenced against (already decoded image bytes), or null
  int32_t n;
};
// One decoder work item: segments first, first + stride, ... (`count` of them), decoded in this
// order by one thread: the same segment of a chain of records differenced against each other.
struct WireUnit {
  int32_t first, stride, count;
};
struct WireSegRef {
  int32_t rec;
  int32_t n;
  int64_t e0;  // first element
};

// Segments and decode units of a run of records (diff[i]: record i is differenced against
// record i - 1, which then has the same element count).
void wire_layout(const int64_t* n_elems, const int32_t* diff, int n_recs, std::vector<WireSegRef>* segs,
                 std::vector<WireUnit>* units);

struct WireJob {
  const char* wire = nullptr;  // table | payload
  int64_t wire_bytes = 0;      // bytes of `wire` that may be read
  const WireSegHost* segs = nullptr;
  int64_t n_seg = 0;
  const WireUnit* units = nullptr;
  int64_t n_units = 0;
  // results
  int status = 0;          // 0, or TK_ERR_INVALID_ARG for a wire buffer that does not parse
  int64_t used_bytes = 0;  // table + segments (each rounded to 64 B)
  double ms = 0.0;
};
// Decodes on the pool (threads <= 0: all of it) and waits; makes no HIP call.
int wire_decode(WireJob* job, int threads);
int wire_pool_threads();

}  // namespace tk
