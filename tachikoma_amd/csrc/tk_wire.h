// Trace wire format: int32 trace records leave the device losslessly narrowed and are widened
// on the host; 1-byte records that are a clamp of the record before them leave as that statement
// and are rebuilt on the host (tk_wire.cc: the planner, host decoder, thread pool and reference
// encoder; tk_trace.hip: the device encoder, the device decoder that verifies and loads trace files
// and their entry points; tk_capture_plan.cc and tk_capture.cc: the packed capture that uses them).
//
// A record of n int32 elements is cut into blocks of kWireBlock elements and segments of
// kWireSegBlocks blocks (the last block / segment of a record may be short).  The coded value of
// an element is the element itself or, for a differenced record, element - predecessor element
// with int32 wrap-around; a differenced record may also carry a per-channel addend (bias coding: a
// bias_add record after its convolution), and then the coded value of element e is
// element - predecessor element - addend[(e / plane) % channels], `plane` being the product of the
// dims after the bias axis and `channels` the dim on it (a dense record has plane 1).  The addend is
// a predictor: encoder and decoder are handed the same values (the packed plan snapshots the bias
// once, a device copy for the encoder and a host copy for the decoder), any values round-trip any
// data, and where they are the bias every block of the record is constant -- also the blocks that
// straddle a plane boundary, which a plain difference pays 1-2 bytes per element for.  Geometry,
// widths, table and cursor are the same with and without an addend.  A block is coded as base (the minimum coded value) plus unsigned
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
//
// 1-byte records (kind int8 / uint8) keep this geometry with one element per byte and two block
// forms each.  A plain record: width 0 is a constant block (the value in byte 0 of the base),
// width 1 one raw plane of the record's own bytes.  A clamp-predicted record (its predecessor is a
// record of the same kind and element count): width 0 means block == clamp(predecessor's block, lo,
// hi), with lo / hi the block's own minimum / maximum compared in the record's dtype and stored in
// base bytes 0 / 1; width 1 is the raw plane (not a residual), the escape of a block the clamp does
// not reproduce.  If rec == clamp(prev, L, H) holds on a block for any L, H then
// clamp(prev, min(rec), max(rec)) reproduces it, so the prediction needs no clip attributes and
// any data round-trips.  Other widths are refused in a 1-byte segment.
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/tachikoma.h"

namespace tk {

constexpr int kWireBlock = 256;
constexpr int kWireSegBlocks = 64;
constexpr int kWireSegElems = kWireBlock * kWireSegBlocks;
// entries one workgroup scans in the packer's prefix sum over the segment sizes (tk_wire_pack_device)
constexpr int kWireScanTile = 2048;

inline int64_t wire_align(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
inline int64_t wire_table_bytes(int64_t n_seg) { return wire_align(4 * n_seg, 64); }
inline int64_t wire_header_bytes(int nb) { return wire_align(4 * (int64_t)nb, 16) + wire_align(nb, 16); }
// element kind of a record / segment (tk_wire_record.kind)
enum WireKind : int32_t { kWireI32 = 0, kWireI8 = 1, kWireU8 = 2, kWireI32Bias = 3 };
// A record of kind kWireI32Bias is an int32 record coded with an addend (tk_wire_addend); its
// segments are int32 segments (kWireI32) that carry the addend.  Packed trace files of format
// version 3 store such records with their addend values; the entry points behind them are
// tk_wire_check_bias, tk_wire_pack_device_bias and tk_wire_unpack_device_bias.
inline int wire_seg_kind(int kind) { return kind == kWireI32Bias ? (int)kWireI32 : kind; }
inline int wire_elem_bytes(int kind) { return wire_seg_kind(kind) == kWireI32 ? 4 : 1; }
// worst case (every block raw) of a segment of n elements of esize bytes
inline int64_t wire_seg_bound(int n, int esize = 4) {
  return wire_align(wire_header_bytes((n + kWireBlock - 1) / kWireBlock) + esize * (int64_t)n, 64);
}

// Where a bias-coded segment starts in its record: element e0 lies in the plane of channel c0 at
// position r0.  Computed on the host, so that the device walks a segment in 32-bit arithmetic.
struct WireSegPos { int32_t c0, r0; };
inline WireSegPos wire_seg_pos(int64_t e0, int32_t plane, int32_t channels) {
  return {(int32_t)((e0 / plane) % channels), (int32_t)(e0 % plane)};
}
// The bias coding of a segment (WireSegDev, WireSegHost; the device decoder's table parallel to WireSegOut).
struct WireBias {
  const int32_t* addend = nullptr;  // `channels` values whoever reads the segment can read; null: no addend
  int32_t plane = 0, channels = 0;
  int32_t c0 = 0, r0 = 0;           // wire_seg_pos of the segment's first element
};
// of a segment that starts at element e0 of a record coded with `addend` (null: none)
inline WireBias wire_seg_bias(const int32_t* addend, int32_t plane, int32_t channels, int64_t e0) {
  if (!addend) return {};
  const WireSegPos at = wire_seg_pos(e0, plane, channels);
  return {addend, plane, channels, at.c0, at.r0};
}

// device encoder's view of a segment
struct WireSegDev {
  const void* src;
  const void* prev;  // differenced against / clamp-predicted from (device), or null
  int32_t n;
  int32_t kind;
  WireBias bias;     // addend on the device
};
// device decoder's view (tk_wire_unpack_device): a segment's destination, and a decode unit
struct WireSegOut {
  void* dst;  // the segment's first element in the record's buffer (device), or null
  int32_t rec;
  int32_t pad;
};
struct WireUnitDev {
  int32_t first, stride, count;  // segments first, first + stride, ...
  int32_t n, kind;               // elements and kind of each of them
  int32_t pad;
  int64_t e0;                    // the segments' first element in their records
};
// one pair of tk_compare_device_batch
struct ComparePair {
  const uint8_t* expected;
  const uint8_t* got;
  int64_t bytes;
  int64_t first_blk;  // first workgroup of this pair in the launch
  int32_t elem_bytes;
  int32_t pad;
};
// host decoder's view: destinations in the trace image, any alignment
struct WireSegHost {
  char* dst;
  const char* prev;  // differenced against / clamp-predicted from (image bytes already present), or null
  int32_t n;
  int32_t kind;
  WireBias bias;     // addend on the host
};
// (the tables uploaded to the device keep their sizes)
static_assert(sizeof(WireBias) == 24 && sizeof(WireSegDev) == 48 && sizeof(WireSegHost) == 48, "wire segment layout");
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

// record i's addend where it has one (kind 3 and addends given), else null
inline const tk_wire_addend* wire_addend_of(const tk_wire_record* recs, const tk_wire_addend* addends, int i) {
  return addends && recs[i].kind == kWireI32Bias ? addends + i : nullptr;
}

// The plan of a run of records: segments, decode units (record i with `diff` is decoded after the
// same segment of record i - 1, which has its kind and element count: differenced against it, or
// clamp-predicted from it) and the wire buffer's size with every block raw.  Segments count elements.
struct WirePlan {
  std::vector<WireSegRef> segs;
  std::vector<WireUnit> units;
  int64_t bound = 0;
};
// Plans `recs` for the entry point `who`, offsets held to an image of image_bytes (-1: not looked
// at).  An unknown kind, a record of no size or outside the image, a `diff` across a change of size
// or kind (kinds 0 and 3 chain with each other), a record of kind 3 that is not differenced, has
// 2^31 elements or more, or whose addends[i] has no addend or a plane or channels below 1, 2^31
// segments or more: sets the error under `who`'s name and returns the status.  `addends` null (every
// entry point without addends; packed trace files of version 2 and their device decoder): kind 3 is refused
// (TK_ERR_UNSUPPORTED) unless `bias_ok` (tk_wire_bound: the size does not depend on the addend).
int wire_plan(const tk_wire_record* recs, int n_recs, int64_t image_bytes, const char* who, WirePlan* plan,
              const tk_wire_addend* addends = nullptr, bool bias_ok = false);

// Where a segment starts in its record's buffer and in its predecessor's (a null base gives null).
// Whether the two are chained in the decode order is the plan's `diff`: another plan may hold the predecessor.
struct WireSegAddr { char* at; const char* prev; };
inline WireSegAddr wire_seg_addr(const WireSegRef& s, int kind, const void* base, const void* prev_base) {
  const int64_t b0 = wire_elem_bytes(kind) * s.e0;
  return {base ? (char*)base + b0 : nullptr, prev_base ? (const char*)prev_base + b0 : nullptr};
}

// The same for a record of an entry point's list: record i's coding where it has an addend, else none.
inline WireBias wire_seg_bias(const tk_wire_record* recs, const tk_wire_addend* addends, int i, int64_t e0) {
  const tk_wire_addend* ad = wire_addend_of(recs, addends, i);
  return ad ? wire_seg_bias(ad->addend, ad->plane, ad->channels, e0) : WireBias{};
}

// Unrounded length of a segment of n elements of `kind` placed at table entry `start`, from the
// widths its header states; -1 if start, header or length leave the payload or a width is not one
// of the kind's (tk_wire.cc).  Reads no block payload.
int64_t wire_seg_extent(int kind, int n, uint32_t start, const char* payload, int64_t payload_bytes);

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
