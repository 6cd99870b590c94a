// The plan of a packed trace capture (tk_capture.cc): which node outputs have host destinations,
// how each leaves the device (gathered into the mirror by the pack kernel, or coded on the trace
// wire: plain, differenced, bias-coded, clamp-predicted), where the image is cut into chunks, and
// the tables the pack kernel, the wire encoder and the host decoder work from.  Host only, no HIP,
// and nothing is allocated on the device: tools/capture_plan_check.cc runs it on a CPU.
#pragma once

#include <stdint.h>

#include <vector>

#include "tk_node.h"
#include "tk_wire.h"

namespace tk {

// One record of the pack kernel's device table (tk_trace.hip: pack_records_kernel).
struct PackRec {
  const uint8_t* src;
  int64_t dst;        // offset in the mirror
  int64_t bytes;
  int64_t first_blk;  // first workgroup of this record in the launch
};
// Workgroups the pack kernel gives a record of `bytes` at mirror offset `dst`: one thread per
// 16-byte aligned chunk of the mirror that the record touches, 256 threads each.
inline int64_t pack_rec_blocks(int64_t dst, int64_t bytes) {
  const int64_t a0 = dst & ~(int64_t)15;
  return (dst + bytes - a0 + 256 * 16 - 1) / (256 * 16);
}

// A record of the plan: a node output that has a host destination.
struct CaptureRecord {
  char* host;
  const void* src;
  int64_t bytes;
  int node, out;
  const tk_tensor* t;
  bool wire, diff;  // coded on the wire; as the difference from the record before it
  bool clamp;       // coded on the wire as a clamp of the record before it (1-byte)
  // a differenced record that is the bias_add of the record before it: the bias vector, the
  // geometry of its axis and where its snapshot lies in the plan's addend buffers (int32 elements)
  const tk_tensor* bias = nullptr;
  int32_t plane = 0, channels = 0;
  int64_t addend_at = 0;
};

// what the module's settings say about a plan
struct CaptureOptions {
  int chunks;  // the image is cut into about this many
  bool wire;   // code records on the trace wire
  bool clamp;  // ... clip records as clamps of their predecessor
  bool bias;   // ... bias_add records as predecessor plus bias
};

struct CapturePlan {
  std::vector<CaptureRecord> recs;  // host order (they point into the node list)
  bool wire = false;                // some record is coded
  char* host_lo = nullptr;          // mirrored host range [host_lo, host_lo + span)
  int64_t span = 0;
  // int32 elements of the addend snapshot: recs[i].channels values of recs[i].bias at
  // recs[i].addend_at, for every record with a bias
  int64_t addend_total = 0;
  struct Chunk {
    int after_node;               // pack + event after this node
    int64_t off, len;             // mirror range copied to host_lo + off
    int64_t table_off;            // first entry in `table`
    int n_rec;
    int64_t blocks;
  };
  std::vector<Chunk> chunks;
  std::vector<PackRec> table;     // the pack table of every chunk
  // Trace wire: the int32 records of a chunk, and its 1-byte records that are clips of the record
  // before them, are not packed; an encode kernel writes them into a pinned slot and a host
  // function widens the slot into the image.
  struct Range {
    int64_t off, len;
  };
  struct WireChunk {
    std::vector<Range> raw;  // mirror ranges of the records that are not coded (runs of adjacent ones)
    int64_t seg_off = 0;     // first entry in `wire_segs`
    int64_t coded_bytes = 0, bound = 0;
    std::vector<WireSegHost> segs;
    std::vector<WireUnit> units;
  };
  std::vector<WireChunk> wchunks;        // one per chunk where `wire`
  std::vector<WireSegDev> wire_segs;     // the encoder's segments of every chunk
};

// Step 1: the records (none: nothing to capture), their coding, the mirrored range and the layout
// of the addend snapshot.  host_dst: TK_MAX_NODE_OUTPUTS entries per node.
int capture_plan_records(const std::vector<Node>& nodes, void* const* host_dst, const CaptureOptions& opt,
                         CapturePlan* plan);
// Step 2: the chunks, cut at node boundaries where every record below the cut is written, with the
// pack table and, on the wire, each chunk's raw ranges and wire tables.  addend_dev / addend_host:
// where the encoder and the decoder will find the snapshot (addend_total elements each; never read here).
int capture_plan_chunks(int n_nodes, int chunks, const int32_t* addend_dev, const int32_t* addend_host,
                        CapturePlan* plan);

}  // namespace tk
