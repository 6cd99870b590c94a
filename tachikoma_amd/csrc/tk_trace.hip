// The trace transport on the device, for gfx950: the kernels that carry trace records to host
// memory and to trace files, and back for verification (record copy, trace image pack, wire encoder,
// the packer's prefix sum, wire decoder, raw compare, digest), then the extern "C" entry points that
// launch them on their own.  The packed capture (tk_capture.cc) launches pack_records_impl and
// wire_encode_impl, the executor's graph copies host_copy_impl (tk_ops.h); all else is file-local.
// tk_wire.h has the wire format, tk_wire.cc the planner and the host codec.
#include <algorithm>
#include <climits>
#include <mutex>
#include <string>
#include <vector>

#include "tk_ops.h"

namespace tk {

// launch geometry of the digest, a grid-stride kernel like tk_elementwise.hip's: ~8 workgroups per CU
constexpr int kBlock = 256;
static inline int grid_for(int64_t work_items) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((work_items + kBlock - 1) / kBlock, 256 * 8));
}

// ---------------------------------------------------------------- records to host memory
// One launch copies up to kHostCopyMax device buffers into pinned host memory (a node's trace
// records; tk_module_run_graph's copies).  Host destinations are 8-byte aligned (NDArray-list
// payloads); each buffer is copied as an 8-byte head (to reach 16-byte destination alignment),
// 16-byte nontemporal stores from two 8-byte loads, and a byte tail.  64-128 workgroups of such a
// kernel write pinned memory at ~55 GB/s (profiles/r03b_probe_d2h.jsonl, kernel_wg128), about the
// SDMA engines' rate, and as a graph kernel node it needs no per-copy host call.
constexpr int kHostCopyMax = 6;
struct HostCopies {
  const uint8_t* src[kHostCopyMax];
  uint8_t* dst[kHostCopyMax];
  int64_t bytes[kHostCopyMax];
  int n;
};

__global__ __launch_bounds__(256) void host_copy_kernel(HostCopies c) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int b = 0; b < c.n; ++b) {
    const uint8_t* src = c.src[b];
    uint8_t* dst = c.dst[b];
    int64_t n = c.bytes[b];
    const int64_t head = (int64_t)((16 - ((uintptr_t)dst & 15)) & 15) < n ? (int64_t)((16 - ((uintptr_t)dst & 15)) & 15) : n;
    for (int64_t i = t; i < head; i += stride) dst[i] = src[i];
    const int64_t n16 = (n - head) / 16;
    const uint64_t* s8 = reinterpret_cast<const uint64_t*>(src + head);
    tk_v4i* d16 = reinterpret_cast<tk_v4i*>(dst + head);
    if (((uintptr_t)(src + head) & 7) == 0) {
      for (int64_t i = t; i < n16; i += stride) {
        const uint64_t a = __builtin_nontemporal_load(s8 + 2 * i), bb = __builtin_nontemporal_load(s8 + 2 * i + 1);
        __builtin_nontemporal_store(tk_v4i{(int)(uint32_t)a, (int)(uint32_t)(a >> 32), (int)(uint32_t)bb, (int)(uint32_t)(bb >> 32)},
                                    d16 + i);
      }
    } else {
      for (int64_t i = t; i < n16 * 16; i += stride) dst[head + i] = src[head + i];
    }
    for (int64_t i = head + n16 * 16 + t; i < n; i += stride) dst[i] = src[i];
  }
}

int host_copy_impl(const void* const* src, void* const* dst, const int64_t* bytes, int n, hipStream_t s) {
  TK_CHECK_ARG(n >= 0 && n <= kHostCopyMax, "host copy: too many buffers");
  HostCopies c{};
  int64_t total = 0;
  int k = 0;
  for (int i = 0; i < n; ++i) {
    if (!dst[i] || bytes[i] <= 0) continue;
    c.src[k] = (const uint8_t*)src[i];
    c.dst[k] = (uint8_t*)dst[i];
    c.bytes[k] = bytes[i];
    total += bytes[i];
    ++k;
  }
  c.n = k;
  if (!k) return TK_OK;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(128, (total / 16 + 255) / 256));
  hipLaunchKernelGGL(host_copy_kernel, dim3(grid), dim3(256), 0, s, c);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// ---------------------------------------------------------------- trace image pack
// Packed trace capture (tk_module_run_graph's default): a chunk's records are gathered from their
// own device buffers into a device mirror of the trace image's records section, at their final
// (NDArray-list, any-alignment) offsets, so that the chunk leaves for host memory as ONE contiguous
// SDMA copy (host-issued copies of whole chunks run at 57.0 GB/s, per-record copies at 56.0 and
// graph memcpy nodes at 54.0-54.6, profiles/r04c_copyprobe.jsonl).  One thread writes one 16-byte
// aligned chunk of the mirror: whole chunks from two aligned 16-byte source loads and a funnel
// shift, partial chunks (next to a header) byte by byte, header bytes left as they are.  Record
// buffers must be 16-byte aligned and readable in whole 16-byte chunks (torch allocations are).
// PackRec, the table entry, and a record's workgroup count: tk_capture_plan.h.
__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t r) {
  return r ? __builtin_amdgcn_alignbyte(hi, lo, r) : lo;
}

__global__ __launch_bounds__(256) void pack_records_kernel(const PackRec* __restrict__ recs, int nrec,
                                                           uint8_t* __restrict__ mirror) {
  int lo = 0, hi = nrec - 1;
  const int64_t b = blockIdx.x;
  while (lo < hi) {  // the record whose workgroups include b
    const int mid = (lo + hi + 1) >> 1;
    if (recs[mid].first_blk <= b) lo = mid;
    else hi = mid - 1;
  }
  const PackRec r = recs[lo];
  const int64_t a0 = r.dst & ~(int64_t)15;  // first 16-byte chunk touching the payload
  const int64_t a = a0 + ((b - r.first_blk) * 256 + threadIdx.x) * 16;
  const int64_t end = r.dst + r.bytes;
  if (a >= end) return;
  if (a >= r.dst && a + 16 <= end) {
    const int64_t so = a - r.dst;  // source offset of the chunk's first byte
    const int64_t base = so & ~(int64_t)15;
    const uint32_t s = (uint32_t)(so - base);
    tk_v4i v0 = __builtin_nontemporal_load(reinterpret_cast<const tk_v4i*>(r.src + base));
    tk_v4i out;
    if (s == 0) {
      out = v0;
    } else {
      tk_v4i v1 = __builtin_nontemporal_load(reinterpret_cast<const tk_v4i*>(r.src + base + 16));
      const uint32_t w[8] = {(uint32_t)v0.x, (uint32_t)v0.y, (uint32_t)v0.z, (uint32_t)v0.w,
                             (uint32_t)v1.x, (uint32_t)v1.y, (uint32_t)v1.z, (uint32_t)v1.w};
      const uint32_t q = s >> 2, rb = s & 3;
      uint32_t o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // w[k + q] / w[k + q + 1] through selects (no dynamic register indexing)
        const uint32_t x0 = q == 0 ? w[k] : q == 1 ? w[k + 1] : q == 2 ? w[k + 2] : w[k + 3];
        const uint32_t x1 = q == 0 ? w[k + 1] : q == 1 ? w[k + 2] : q == 2 ? w[k + 3] : w[k + 4];
        o[k] = funnel(x0, x1, rb);
      }
      out = tk_v4i{(int)o[0], (int)o[1], (int)o[2], (int)o[3]};
    }
    *reinterpret_cast<tk_v4i*>(mirror + a) = out;
  } else {
    const int64_t from = a > r.dst ? a : r.dst;
    const int64_t to = a + 16 < end ? a + 16 : end;
    for (int64_t i = from; i < to; ++i) mirror[i] = r.src[i - r.dst];
  }
}

int pack_records_impl(const PackRec* table, int nrec, int64_t blocks, void* mirror, hipStream_t s) {
  TK_CHECK_ARG(table && mirror && nrec > 0 && blocks > 0, "bad arguments");
  hipLaunchKernelGGL(pack_records_kernel, dim3((unsigned)blocks), dim3(256), 0, s, table, nrec, (uint8_t*)mirror);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// ---------------------------------------------------------------- trace wire encoder
// The device side of the wire format (tk_wire.h): one workgroup codes one segment of up to 64
// blocks of 256 int32 elements, read from the record's own device buffer (minus the predecessor
// record's element for a differenced record).  16 lanes own a block, 16 consecutive elements
// each, so a block's minimum and maximum are a 16-lane butterfly and a lane's share of a byte
// plane is exactly one 16-byte store; the workgroup's 16 lane groups take four passes over the
// segment, keeping the 64 offsets of a thread in registers.  After the widths are known one
// thread takes the segment's place from the buffer's cursor (units of 64 B) and publishes it in
// the table at the front of the buffer; nothing is stored if the place would end past `cap_units`
// (it cannot: the buffer is sized for every block raw), and the decoder then refuses the entry.
// The buffer is usually a pinned host slot: every store to it is a full 16-byte plane piece, a
// header word, or (last, short block of a record only) a byte.
//
// 1-byte segments (kind int8 / uint8) keep the geometry: a lane's 16 elements are one 16-byte load
// of the record and, for a clamp-predicted record, one of its predecessor.  Bytes are compared as
// uint8 (int8 with the sign bit flipped); the butterfly gives the block's lo and hi, every lane
// tests clamp(prev, lo, hi) == src on its 16 bytes and a 16-lane AND decides between width 0 and
// the raw plane, which is the lane's 16 loaded bytes stored as they are.
//
// Bias coding (an int32 segment with an addend): after the predecessor, a lane subtracts from each
// of its 16 values the addend of that element's channel.  The segment's first element lies at
// position r0 of channel c0's plane (host-computed), so the lane's first one, e0 elements on, is
// found with one 32-bit division; from there the walk steps position and channel per element and
// reloads the addend only where the channel changes (a lane crosses several planes where plane < 16).
// The channel is always one of the addend's, so the walk may run past the record's end.
__device__ __forceinline__ uint32_t wire_byte(const uint32_t* w, int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xFFu; }

__device__ __forceinline__ void wire_sub_addend(uint32_t* x, const WireBias& wb, int e0) {
  const uint32_t plane = (uint32_t)wb.plane, channels = (uint32_t)wb.channels;
  const uint32_t t = (uint32_t)wb.r0 + (uint32_t)e0;
  const uint32_t q = t / plane;
  uint32_t r = t - q * plane;
  uint32_t c = ((uint32_t)wb.c0 + q) % channels;
  uint32_t a = (uint32_t)wb.addend[c];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    x[j] -= a;
    if (++r == plane) {
      r = 0;
      c = c + 1 == channels ? 0 : c + 1;
      a = (uint32_t)wb.addend[c];
    }
  }
}

// The packer of trace files (tk_wire_pack_device) runs the same code twice around a prefix sum, so
// that segment i lies where the host encoder puts it whatever order the workgroups finish in:
// kWireSize stops once the widths are known and writes the segment's size in 64-byte units to
// table[i]; kWirePlace reads the segment's start from table[i] (the scanned sizes) instead of taking
// it from the cursor and also zeroes the segment's tail up to 64 B.  kWireCursor is the live wire.
enum { kWireCursor = 0, kWireSize = 1, kWirePlace = 2 };

template <int kMode>
__global__ __launch_bounds__(256) void wire_encode_kernel(const WireSegDev* __restrict__ segs, uint32_t* cursor,
                                                          uint32_t* __restrict__ table, uint8_t* __restrict__ payload,
                                                          uint32_t cap_units) {
  __shared__ int32_t s_base[kWireSegBlocks];
  __shared__ uint32_t s_w[kWireSegBlocks];
  __shared__ uint32_t s_off[kWireSegBlocks];
  __shared__ uint32_t s_start;
  const WireSegDev sg = segs[blockIdx.x];
  const int n = sg.n;
  const int nb = (n + kWireBlock - 1) / kWireBlock;
  const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
  const bool aligned = ((((uintptr_t)sg.src) | ((uintptr_t)sg.prev)) & 15) == 0;
  const bool bytes = sg.kind != kWireI32;
  const int32_t* src32 = static_cast<const int32_t*>(sg.src);
  const int32_t* prev32 = static_cast<const int32_t*>(sg.prev);
  uint32_t v[4][16];  // 1-byte segments: v[p][0..3] are the lane's 16 bytes as loaded
  if (bytes) {
    const uint8_t* src8 = static_cast<const uint8_t*>(sg.src);
    const uint8_t* prev8 = static_cast<const uint8_t*>(sg.prev);
    const uint32_t flip = sg.kind == kWireI8 ? 0x80u : 0u;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int b = p * 16 + g;
      const int e0 = b * kWireBlock + l * 16;
      const int valid = min(16, n - e0);  // <= 0: the lane holds nothing
      uint32_t pv[4] = {0, 0, 0, 0};
      if (aligned && valid == 16) {
        const tk_v4i a = *reinterpret_cast<const tk_v4i*>(src8 + e0);
        v[p][0] = (uint32_t)a.x, v[p][1] = (uint32_t)a.y, v[p][2] = (uint32_t)a.z, v[p][3] = (uint32_t)a.w;
        if (prev8) {
          const tk_v4i c = *reinterpret_cast<const tk_v4i*>(prev8 + e0);
          pv[0] = (uint32_t)c.x, pv[1] = (uint32_t)c.y, pv[2] = (uint32_t)c.z, pv[3] = (uint32_t)c.w;
        }
      } else {
        v[p][0] = v[p][1] = v[p][2] = v[p][3] = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (j < valid) {
            v[p][j >> 2] |= (uint32_t)src8[e0 + j] << (8 * (j & 3));
            if (prev8) pv[j >> 2] |= (uint32_t)prev8[e0 + j] << (8 * (j & 3));
          }
      }
      uint32_t lo = 0xFFu, hi = 0u;  // in the flipped (unsigned) order
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (j < valid) {
          const uint32_t x = wire_byte(v[p], j) ^ flip;
          lo = min(lo, x), hi = max(hi, x);
        }
#pragma unroll
      for (int m = 8; m >= 1; m >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, m, 16));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, m, 16));
      }
      int coded = 0;
      if (prev8) {  // the same for the whole workgroup: every lane takes part in the AND
        coded = 1;
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (j < valid) coded &= min(max(wire_byte(pv, j) ^ flip, lo), hi) == (wire_byte(v[p], j) ^ flip);
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) coded &= __shfl_xor(coded, m, 16);
      }
      coded |= lo == hi;
      if (l == 0 && b < nb) s_base[b] = (int32_t)((lo ^ flip) | ((hi ^ flip) << 8)), s_w[b] = coded ? 0u : 1u;
    }
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int b = p * 16 + g;
      const int e0 = b * kWireBlock + l * 16;
      int32_t mn = INT_MAX, mx = INT_MIN;
      if (aligned && e0 + 16 <= n) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const tk_v4i a = *reinterpret_cast<const tk_v4i*>(src32 + e0 + 4 * q);
          v[p][4 * q] = (uint32_t)a.x, v[p][4 * q + 1] = (uint32_t)a.y, v[p][4 * q + 2] = (uint32_t)a.z,
                   v[p][4 * q + 3] = (uint32_t)a.w;
        }
        if (prev32) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const tk_v4i a = *reinterpret_cast<const tk_v4i*>(prev32 + e0 + 4 * q);
            v[p][4 * q] -= (uint32_t)a.x, v[p][4 * q + 1] -= (uint32_t)a.y, v[p][4 * q + 2] -= (uint32_t)a.z,
                v[p][4 * q + 3] -= (uint32_t)a.w;
          }
        }
        if (sg.bias.addend) wire_sub_addend(v[p], sg.bias, e0);
#pragma unroll
        for (int j = 0; j < 16; ++j) mn = min(mn, (int32_t)v[p][j]), mx = max(mx, (int32_t)v[p][j]);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          uint32_t x = 0;
          if (e0 + j < n) {
            x = (uint32_t)src32[e0 + j];
            if (prev32) x -= (uint32_t)prev32[e0 + j];
          }
          v[p][j] = x;
        }
        // (the walk also passes over the elements past the record's end: they are never stored)
        if (sg.bias.addend && e0 < n) wire_sub_addend(v[p], sg.bias, e0);
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (e0 + j < n) mn = min(mn, (int32_t)v[p][j]), mx = max(mx, (int32_t)v[p][j]);
      }
#pragma unroll
      for (int m = 8; m >= 1; m >>= 1) {
        mn = min(mn, __shfl_xor(mn, m, 16));
        mx = max(mx, __shfl_xor(mx, m, 16));
      }
      // exact in unsigned arithmetic (mx >= mn as signed values): INT_MIN and INT_MAX in one block
      // give 2^32 - 1 and the raw width, not a wrapped range
      const uint32_t range = (uint32_t)mx - (uint32_t)mn;
      const uint32_t w = range == 0 ? 0 : range <= 0xFFu ? 1 : range <= 0xFFFFu ? 2 : range <= 0xFFFFFFu ? 3 : 4;
      if (l == 0 && b < nb) s_base[b] = mn, s_w[b] = w;
#pragma unroll
      for (int j = 0; j < 16; ++j) v[p][j] -= (uint32_t)mn;
    }
  }
  __syncthreads();
  const uint32_t base_bytes = (uint32_t)((4 * nb + 15) & ~15);
  const uint32_t hdr = base_bytes + (uint32_t)((nb + 15) & ~15);
  if (threadIdx.x == 0) {
    uint32_t off = hdr;
    for (int b = 0; b < nb; ++b) {
      s_off[b] = off;
      off += s_w[b] * (uint32_t)min(kWireBlock, n - b * kWireBlock);
    }
    const uint32_t units = (off + 63) >> 6;
    if constexpr (kMode == kWireSize) {
      table[blockIdx.x] = units;
      return;
    }
    const uint32_t start = kMode == kWirePlace ? table[blockIdx.x] : atomicAdd(cursor, units);
    if constexpr (kMode == kWireCursor) table[blockIdx.x] = start;
    s_start = start <= cap_units && units <= cap_units - start ? start : 0xFFFFFFFFu;
  }
  if constexpr (kMode == kWireSize) return;
  __syncthreads();
  if (s_start == 0xFFFFFFFFu) return;
  uint8_t* out = payload + (uint64_t)s_start * 64;
  // header: bases as words, widths four to a word (the padding of both parts written as zeros)
  if ((int)threadIdx.x < (int)(base_bytes >> 2))
    reinterpret_cast<int32_t*>(out)[threadIdx.x] = (int)threadIdx.x < nb ? s_base[threadIdx.x] : 0;
  if ((int)threadIdx.x < (int)((hdr - base_bytes) >> 2)) {
    uint32_t ww = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = (int)threadIdx.x * 4 + j;
      if (b < nb) ww |= s_w[b] << (8 * j);
    }
    reinterpret_cast<uint32_t*>(out + base_bytes)[threadIdx.x] = ww;
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int b = p * 16 + g;
    if (b >= nb) continue;
    const int cnt = min(kWireBlock, n - b * kWireBlock);
    const uint32_t w = s_w[b];
    uint8_t* q = out + s_off[b];
    if (bytes) {
      if (w == 0) continue;
      if (cnt == kWireBlock) {
        __builtin_nontemporal_store(tk_v4i{(int)v[p][0], (int)v[p][1], (int)v[p][2], (int)v[p][3]},
                                    reinterpret_cast<tk_v4i*>(q + l * 16));
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (l * 16 + j < cnt) q[l * 16 + j] = (uint8_t)wire_byte(v[p], j);
      }
      continue;
    }
    for (uint32_t k = 0; k < w; ++k) {
      const uint32_t sh = 8 * k;
      uint32_t o[4];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        o[c] = ((v[p][4 * c] >> sh) & 0xFFu) | (((v[p][4 * c + 1] >> sh) & 0xFFu) << 8) |
               (((v[p][4 * c + 2] >> sh) & 0xFFu) << 16) | (((v[p][4 * c + 3] >> sh) & 0xFFu) << 24);
      if (cnt == kWireBlock) {
        __builtin_nontemporal_store(tk_v4i{(int)o[0], (int)o[1], (int)o[2], (int)o[3]},
                                    reinterpret_cast<tk_v4i*>(q + k * kWireBlock + l * 16));
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (l * 16 + j < cnt) q[k * cnt + l * 16 + j] = (uint8_t)(o[j >> 2] >> (8 * (j & 3)));
      }
    }
  }
  if constexpr (kMode == kWirePlace) {
    // the tail: fewer than 64 bytes, none of them a plane's
    const uint32_t end = s_off[nb - 1] + s_w[nb - 1] * (uint32_t)(n - (nb - 1) * kWireBlock);
    const uint32_t at = end + threadIdx.x;
    if (at < ((end + 63) & ~63u)) out[at] = 0;
  }
}

int wire_encode_impl(const WireSegDev* segs, int64_t n_seg, uint32_t* cursor, void* wire, int64_t wire_bytes,
                     hipStream_t s) {
  const int64_t table = wire_table_bytes(n_seg);
  TK_CHECK_ARG(segs && cursor && wire && n_seg > 0 && n_seg < ((int64_t)1 << 31) && ((uintptr_t)wire & 63) == 0 &&
               wire_bytes >= table, "bad arguments");
  const int64_t cap_units = std::min<int64_t>((wire_bytes - table) / 64, 0xFFFFFFF0ll);
  hipLaunchKernelGGL(wire_encode_kernel<kWireCursor>, dim3((unsigned)n_seg), dim3(256), 0, s, segs, cursor, (uint32_t*)wire,
                     (uint8_t*)wire + table, (uint32_t)cap_units);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// ---------------------------------------------------------------- trace file packer
// tk_wire_pack_device: the wire format with segment i where the host encoder puts it, so that the
// same records give the same bytes on every run and the length is known before the copy.  Three
// steps, none of which waits for another workgroup: the size pass leaves every segment's size (64-byte
// units) in the table, an exclusive prefix sum turns the table into the starts, the place pass
// stores the segments there.
//
// The prefix sum works on tiles of kWireScanTile entries, one workgroup each, eight consecutive
// entries to a thread: a tile is scanned on its own (in place) and its total goes to the next level,
// which is scanned the same way until a level is a single tile; then each level's offsets are added
// to the tiles of the level below, top down.  A segment is at most 1030 units, so a tile's own sums
// fit 32 bits; the levels above and the grand total are 64-bit, and the caller refuses a total that
// does not fit the table's u32 before anything is placed.
constexpr int kWireScanItems = kWireScanTile / 256;

// v[i] <- v[tile start] + ... + v[i - 1] within each tile of n entries; sums[tile] <- the tile's total
template <typename T>
__global__ __launch_bounds__(256) void wire_scan_tile_kernel(T* v, uint64_t* __restrict__ sums, int64_t n) {
  __shared__ uint64_t s_sum[256];
  const int t = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * kWireScanTile + (int64_t)t * kWireScanItems;
  T x[kWireScanItems];
  uint64_t mine = 0;
#pragma unroll
  for (int j = 0; j < kWireScanItems; ++j) {
    x[j] = i0 + j < n ? v[i0 + j] : (T)0;
    mine += x[j];
  }
  s_sum[t] = mine;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const uint64_t below = t >= d ? s_sum[t - d] : 0;
    __syncthreads();
    s_sum[t] += below;
    __syncthreads();
  }
  uint64_t at = s_sum[t] - mine;
#pragma unroll
  for (int j = 0; j < kWireScanItems; ++j) {
    if (i0 + j < n) v[i0 + j] = (T)at;
    at += x[j];
  }
  if (t == 255) sums[blockIdx.x] = s_sum[255];
}

// v[i] += offs[tile of i]
template <typename T>
__global__ __launch_bounds__(256) void wire_scan_add_kernel(T* __restrict__ v, const uint64_t* __restrict__ offs, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] += (T)offs[i / kWireScanTile];
}

// The entry counts of the scan's levels: [0] the table, then the tile totals of the level below,
// down to a level of one entry, which ends up holding the grand total.
static std::vector<int64_t> wire_scan_levels(int64_t n_seg) {
  std::vector<int64_t> cnt{n_seg};
  do cnt.push_back((cnt.back() + kWireScanTile - 1) / kWireScanTile);
  while (cnt.back() > 1);
  return cnt;
}

static int64_t wire_scan_words(int64_t n_seg) {
  int64_t words = 0;
  const std::vector<int64_t> cnt = wire_scan_levels(n_seg);
  for (size_t k = 1; k < cnt.size(); ++k) words += cnt[k];
  return words;
}

// Sizes and starts: on return (in stream order) table[i] is segment i's start in units and
// scan[wire_scan_words(n_seg) - 1] the units of all segments.  `scan`: wire_scan_words u64 words.
static int wire_pack_plan_impl(const WireSegDev* segs, int64_t n_seg, void* wire, uint64_t* scan, hipStream_t s) {
  TK_CHECK_ARG(segs && wire && scan && n_seg > 0 && n_seg < ((int64_t)1 << 31) && ((uintptr_t)wire & 63) == 0,
               "bad arguments");
  const std::vector<int64_t> cnt = wire_scan_levels(n_seg);
  const int top = (int)cnt.size() - 1;
  std::vector<uint64_t*> lev(cnt.size(), nullptr);
  for (int k = 1; k <= top; ++k) lev[k] = k == 1 ? scan : lev[k - 1] + cnt[k - 1];
  uint32_t* table = (uint32_t*)wire;
  TK_HIP(hipMemsetAsync(wire, 0, (size_t)wire_table_bytes(n_seg), s));
  hipLaunchKernelGGL(wire_encode_kernel<kWireSize>, dim3((unsigned)n_seg), dim3(256), 0, s, segs, (uint32_t*)nullptr, table,
                     (uint8_t*)nullptr, 0u);
  TK_LAUNCH_CHECK();
  hipLaunchKernelGGL(wire_scan_tile_kernel<uint32_t>, dim3((unsigned)cnt[1]), dim3(256), 0, s, table, lev[1], n_seg);
  TK_LAUNCH_CHECK();
  for (int k = 1; k < top; ++k) {
    hipLaunchKernelGGL(wire_scan_tile_kernel<uint64_t>, dim3((unsigned)cnt[k + 1]), dim3(256), 0, s, lev[k], lev[k + 1],
                       cnt[k]);
    TK_LAUNCH_CHECK();
  }
  for (int k = top - 2; k >= 1; --k) {
    hipLaunchKernelGGL(wire_scan_add_kernel<uint64_t>, dim3((unsigned)((cnt[k] + 255) / 256)), dim3(256), 0, s, lev[k],
                       lev[k + 1], cnt[k]);
    TK_LAUNCH_CHECK();
  }
  if (top >= 2) {
    hipLaunchKernelGGL(wire_scan_add_kernel<uint32_t>, dim3((unsigned)((n_seg + 255) / 256)), dim3(256), 0, s, table,
                       lev[1], n_seg);
    TK_LAUNCH_CHECK();
  }
  return TK_OK;
}

// Stores every segment at the start the table states (wire_pack_plan_impl); wire_bytes bounds the stores.
static int wire_pack_place_impl(const WireSegDev* segs, int64_t n_seg, void* wire, int64_t wire_bytes, hipStream_t s) {
  const int64_t table = wire_table_bytes(n_seg);
  TK_CHECK_ARG(segs && wire && n_seg > 0 && n_seg < ((int64_t)1 << 31) && ((uintptr_t)wire & 63) == 0 &&
               wire_bytes >= table, "bad arguments");
  const int64_t cap_units = std::min<int64_t>((wire_bytes - table) / 64, 0xFFFFFFF0ll);
  hipLaunchKernelGGL(wire_encode_kernel<kWirePlace>, dim3((unsigned)n_seg), dim3(256), 0, s, segs, (uint32_t*)nullptr,
                     (uint32_t*)wire, (uint8_t*)wire + table, (uint32_t)cap_units);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// ---------------------------------------------------------------- trace wire decoder
// tk_wire_unpack_device: the way back in.  One workgroup owns a decode unit (tk_wire.h, WireUnit):
// the same segment index of a chain of records linked by `diff`, walked in order.  The geometry is
// the encoder's: 16 lanes own a block and 16 consecutive elements each, the 16 lane groups take
// four passes over the segment's 64 blocks, and a lane's share of a full block's byte plane is one
// 16-byte load.  Every segment's start comes from the table (segments may lie in any order: the
// live encoder places them in completion order); the offsets of its block payloads come from the
// widths by a prefix sum over the (<= 64) blocks, taken by the first wavefront and left in LDS.
//
// The decoded record stays in the registers it was decoded into (v[4][16]: a thread's 64 int32
// values, or its 64 bytes as loaded in v[p][0..3]) and is the next record's predecessor: the int32
// value the difference is added to, or the 16 bytes clamp(prev, lo, hi) is taken of (lo / hi from
// base bytes 0 / 1, int8 through the sign-bit flip).  It is never read back from `dst`: in compare
// mode `dst` holds the data under test, and a wrong record must not make the record chained to it
// look wrong too.  A segment whose `dst` is null is decoded for the chain's sake only.
//
// kStore writes the records (16-byte stores; the short last block of a record and a destination
// that is not 16-byte aligned go element by element) and uses no atomics.  kCompare loads the
// destination's 16 elements instead and counts the elements that differ; the counts are reduced in
// the workgroup, and only a workgroup that found one issues an atomicAdd on the record's count and
// a 64-bit atomicMin on its first differing element, so an equal trace costs no atomic at all.  No
// workgroup waits for another in either mode.
//
// kBias (tk_wire_unpack_device_bias, packed trace files of version 3): a table parallel to `segs`
// gives each segment of a bias-coded record its addend (device), plane, channels and the host's
// wire_seg_pos, and such a segment's element is predecessor + addend[channel] + base + offset.  The
// two instantiations without it are compiled as before the switch existed.
//
// The host refuses a wire buffer tk_wire_check does not accept before it is uploaded; all the same a
// workgroup holds every segment to wire_seg_extent's rules (start, header and stated length inside
// the payload, widths the kind has) before it reads a header or a plane, and on failure sets the
// status word and stores and compares nothing more of its unit.
enum { kWireStore = 0, kWireCompare = 1 };

// (wire_report_mismatches, the workgroup's reduction and its two atomics, is in tk_common.h: the chain
// check reports the same way)

template <int kMode, bool kBias>
__global__ __launch_bounds__(256) void wire_decode_kernel(const WireUnitDev* __restrict__ units,
                                                          const WireSegOut* __restrict__ segs,
                                                          const WireBias* __restrict__ bias,
                                                          const uint32_t* __restrict__ table,
                                                          const uint8_t* __restrict__ payload, int64_t payload_bytes,
                                                          tk_wire_mismatch* report, uint32_t* status) {
  __shared__ int32_t s_base[kWireSegBlocks];
  __shared__ uint32_t s_w[kWireSegBlocks];
  __shared__ uint32_t s_off[kWireSegBlocks];
  __shared__ uint32_t s_bad;
  __shared__ uint32_t s_any[4];
  __shared__ unsigned long long s_red[8];
  const WireUnitDev un = units[blockIdx.x];
  const int n = un.n;
  const int nb = (n + kWireBlock - 1) / kWireBlock;
  const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
  const bool bytes = un.kind != kWireI32;
  const uint32_t max_w = bytes ? 1u : 4u;
  const uint32_t flip = un.kind == kWireI8 ? 0x80u : 0u;
  const uint32_t base_bytes = (uint32_t)((4 * nb + 15) & ~15);
  const uint32_t hdr = base_bytes + (uint32_t)((nb + 15) & ~15);
  uint32_t v[4][16];  // the decoded record (1-byte kinds: v[p][0..3] hold the lane's 16 bytes)
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int j = 0; j < 16; ++j) v[p][j] = 0;
  for (int m = 0; m < un.count; ++m) {
    const int64_t si = un.first + (int64_t)m * un.stride;
    const int64_t off = (int64_t)table[si] * 64;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();  // also: the last record's readers of s_base / s_w / s_off are done
    // start and header inside the payload, before any header byte is read (the same for every thread)
    const bool head_ok = off <= payload_bytes && (int64_t)hdr <= payload_bytes - off;
    const uint8_t* seg = payload + off;
    if (head_ok && threadIdx.x < 64) {  // the first wavefront: widths, bases, prefix sum
      const int b = threadIdx.x;
      uint32_t w = 0, x = 0;
      if (b < nb) {
        w = seg[base_bytes + b];
        s_base[b] = *reinterpret_cast<const int32_t*>(seg + 4 * b);
        s_w[b] = w;
        if (w > max_w) s_bad = 1, w = 0;
        x = w * (uint32_t)min(kWireBlock, n - b * kWireBlock);
      }
      uint32_t incl = x;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, d, 64);
        if (b >= d) incl += y;
      }
      if (b < nb) s_off[b] = hdr + incl - x;
      // the stated length (at most 64 * 4 * 256 + hdr: no overflow) against what is left of the payload
      if (b == 63 && (int64_t)(hdr + incl) > payload_bytes - off) s_bad = 1;
    }
    __syncthreads();
    if (!head_ok || s_bad) {  // the same for every thread
      if (threadIdx.x == 0) *status = 1;
      return;
    }
    const WireSegOut so = segs[si];
    WireBias sb{};
    if constexpr (kBias) sb = bias[si];
    const uint64_t e_seg = (uint64_t)un.e0;
    uint32_t mis = 0, first = 0xFFFFFFFFu;  // the first differing element, counted within the segment
    if (bytes) {
      uint8_t* dst8 = static_cast<uint8_t*>(so.dst);
      const bool aligned = ((uintptr_t)dst8 & 15) == 0;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int b = p * 16 + g;
        if (b >= nb) continue;
        const int cnt = min(kWireBlock, n - b * kWireBlock);
        const int e0 = b * kWireBlock + l * 16;
        const int valid = min(16, n - e0);  // <= 0: the lane holds nothing
        const uint32_t lo = (uint32_t)s_base[b] & 0xFFu, hi = ((uint32_t)s_base[b] >> 8) & 0xFFu;
        if (s_w[b]) {  // the raw plane
          const uint8_t* q = seg + s_off[b];
          if (cnt == kWireBlock) {
            const tk_v4i a = __builtin_nontemporal_load(reinterpret_cast<const tk_v4i*>(q + l * 16));
            v[p][0] = (uint32_t)a.x, v[p][1] = (uint32_t)a.y, v[p][2] = (uint32_t)a.z, v[p][3] = (uint32_t)a.w;
          } else {
            v[p][0] = v[p][1] = v[p][2] = v[p][3] = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j)
              if (j < valid) v[p][j >> 2] |= (uint32_t)q[l * 16 + j] << (8 * (j & 3));
          }
        } else if (m > 0) {  // clamp of the predecessor, which v[p] still holds
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            uint32_t o = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const uint32_t x = ((v[p][c] >> (8 * k)) & 0xFFu) ^ flip;
              o |= (min(max(x, lo ^ flip), hi ^ flip) ^ flip) << (8 * k);
            }
            v[p][c] = o;
          }
        } else {  // a constant block
          v[p][0] = v[p][1] = v[p][2] = v[p][3] = lo * 0x01010101u;
        }
        if (!dst8 || valid <= 0) continue;
        if (aligned && valid == 16) {
          tk_v4i* d = reinterpret_cast<tk_v4i*>(dst8 + e0);
          if constexpr (kMode == kWireStore) {
            *d = tk_v4i{(int)v[p][0], (int)v[p][1], (int)v[p][2], (int)v[p][3]};
          } else {
            const tk_v4i a = *d;
            const uint32_t got[4] = {(uint32_t)a.x, (uint32_t)a.y, (uint32_t)a.z, (uint32_t)a.w};
            if (got[0] != v[p][0] || got[1] != v[p][1] || got[2] != v[p][2] || got[3] != v[p][3]) {
#pragma unroll
              for (int j = 15; j >= 0; --j)
                if (wire_byte(got, j) != wire_byte(v[p], j)) ++mis, first = min(first, (uint32_t)(e0 + j));
            }
          }
        } else {
#pragma unroll
          for (int j = 15; j >= 0; --j) {
            if (j >= valid) continue;
            if constexpr (kMode == kWireStore) dst8[e0 + j] = (uint8_t)wire_byte(v[p], j);
            else if (dst8[e0 + j] != (uint8_t)wire_byte(v[p], j)) ++mis, first = min(first, (uint32_t)(e0 + j));
          }
        }
      }
    } else {
      int32_t* dst32 = static_cast<int32_t*>(so.dst);
      const bool aligned = ((uintptr_t)dst32 & 15) == 0;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int b = p * 16 + g;
        if (b >= nb) continue;
        const int cnt = min(kWireBlock, n - b * kWireBlock);
        const int e0 = b * kWireBlock + l * 16;
        const int valid = min(16, n - e0);
        const uint32_t w = s_w[b];
        const uint8_t* q = seg + s_off[b];
        uint32_t c[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) c[j] = 0;
        for (uint32_t k = 0; k < w; ++k) {
          uint32_t o[4] = {0, 0, 0, 0};
          if (cnt == kWireBlock) {
            const tk_v4i a = __builtin_nontemporal_load(reinterpret_cast<const tk_v4i*>(q + k * kWireBlock + l * 16));
            o[0] = (uint32_t)a.x, o[1] = (uint32_t)a.y, o[2] = (uint32_t)a.z, o[3] = (uint32_t)a.w;
          } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
              if (j < valid) o[j >> 2] |= (uint32_t)q[k * cnt + l * 16 + j] << (8 * (j & 3));
          }
#pragma unroll
          for (int j = 0; j < 16; ++j) c[j] |= wire_byte(o, j) << (8 * k);
        }
        const uint32_t base = (uint32_t)s_base[b];
        bool walked = false;
        if constexpr (kBias) {
          // sb is the same for every thread.  The addend goes in with the base, in the one pass
          // over the lane's 16 values, so no second array of them is live; the walk is
          // wire_sub_addend's (it may pass the record's end, the channel stays one of the addend's)
          if (sb.addend && m > 0) {
            walked = true;
            const uint32_t plane = (uint32_t)sb.plane, channels = (uint32_t)sb.channels;
            const uint32_t t = (uint32_t)sb.r0 + (uint32_t)e0;
            const uint32_t q = t / plane;
            uint32_t r = t - q * plane;
            uint32_t ch = ((uint32_t)sb.c0 + q) % channels;
            uint32_t a = (uint32_t)sb.addend[ch] + base;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
              v[p][j] += a + c[j];  // int32 wrap-around
              if (++r == plane) {
                r = 0;
                ch = ch + 1 == channels ? 0 : ch + 1;
                a = (uint32_t)sb.addend[ch] + base;
              }
            }
          }
        }
        if (!walked) {
#pragma unroll
          for (int j = 0; j < 16; ++j) v[p][j] = (m > 0 ? v[p][j] : 0u) + base + c[j];  // int32 wrap-around
        }
        if (!dst32 || valid <= 0) continue;
        if (aligned && valid == 16) {
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) {
            tk_v4i* d = reinterpret_cast<tk_v4i*>(dst32 + e0 + 4 * q4);
            if constexpr (kMode == kWireStore) {
              *d = tk_v4i{(int)v[p][4 * q4], (int)v[p][4 * q4 + 1], (int)v[p][4 * q4 + 2], (int)v[p][4 * q4 + 3]};
            } else {
              const tk_v4i a = *d;
              const uint32_t got[4] = {(uint32_t)a.x, (uint32_t)a.y, (uint32_t)a.z, (uint32_t)a.w};
#pragma unroll
              for (int j = 3; j >= 0; --j)
                if (got[j] != v[p][4 * q4 + j])
                  ++mis, first = min(first, (uint32_t)(e0 + 4 * q4 + j));
            }
          }
        } else {
#pragma unroll
          for (int j = 15; j >= 0; --j) {
            if (j >= valid) continue;
            if constexpr (kMode == kWireStore) dst32[e0 + j] = (int32_t)v[p][j];
            else if ((uint32_t)dst32[e0 + j] != v[p][j]) ++mis, first = min(first, (uint32_t)(e0 + j));
          }
        }
      }
    }
    if constexpr (kMode == kWireCompare) {
      // so.dst is the same for every thread: all of them take part, or none
      if (so.dst)
        wire_report_mismatches(mis, first == 0xFFFFFFFFu ? ~0ull : (unsigned long long)(e_seg + first), report + so.rec,
                               s_any, s_red);
    }
  }
}

__global__ __launch_bounds__(256) void wire_report_init_kernel(tk_wire_mismatch* report, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) report[i].mismatches = 0, report[i].first = ~0ull;
}

// Resets `report` (device, n entries) on `s`: no mismatch, first = ~0.
int wire_report_init(tk_wire_mismatch* report, int n, hipStream_t s) {
  hipLaunchKernelGGL(wire_report_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, report, n);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// `report` (device, n_report entries) is reset on the stream first; `status` (device) must be zero.
template <int kMode, bool kBias>
static void wire_decode_launch(const void* units, int64_t n_units, const void* segs, const void* bias, const void* wire,
                               int64_t table, int64_t wire_bytes, tk_wire_mismatch* report, uint32_t* status,
                               hipStream_t s) {
  hipLaunchKernelGGL((wire_decode_kernel<kMode, kBias>), dim3((unsigned)n_units), dim3(256), 0, s,
                     (const WireUnitDev*)units, (const WireSegOut*)segs, (const WireBias*)bias, (const uint32_t*)wire,
                     (const uint8_t*)wire + table, wire_bytes - table, report, status);
}

// `bias` (device, a WireBias per segment) selects the instantiations that know addends; null: none.
static int wire_unpack_impl(const void* units, int64_t n_units, const void* segs, const void* bias, const void* wire,
                            int64_t n_seg, int64_t wire_bytes, int mode, tk_wire_mismatch* report, int n_report,
                            uint32_t* status, hipStream_t s) {
  const int64_t table = wire_table_bytes(n_seg);
  TK_CHECK_ARG(units && segs && wire && status && n_units > 0 && n_units < ((int64_t)1 << 31) &&
               ((uintptr_t)wire & 63) == 0 && wire_bytes >= table && (mode == kWireStore || (report && n_report > 0)),
               "bad arguments");
  if (mode == kWireStore) {
    if (bias) wire_decode_launch<kWireStore, true>(units, n_units, segs, bias, wire, table, wire_bytes, nullptr, status, s);
    else wire_decode_launch<kWireStore, false>(units, n_units, segs, nullptr, wire, table, wire_bytes, nullptr, status, s);
  } else {
    hipLaunchKernelGGL(wire_report_init_kernel, dim3((unsigned)((n_report + 255) / 256)), dim3(256), 0, s, report, n_report);
    TK_LAUNCH_CHECK();
    if (bias) wire_decode_launch<kWireCompare, true>(units, n_units, segs, bias, wire, table, wire_bytes, report, status, s);
    else wire_decode_launch<kWireCompare, false>(units, n_units, segs, nullptr, wire, table, wire_bytes, report, status, s);
  }
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// ---------------------------------------------------------------- raw compare
// tk_compare_device: what the wire does not code (float32 / int16 / int64 records, version-1 files,
// params) compared byte for byte, counted in elements.  One thread takes 16 bytes of a pair of
// buffers: one 16-byte load of each where both pointers are 16-byte aligned, four dword loads where
// both are 4-byte aligned, else (and for the pair's tail) byte loads; the mask of differing bytes
// becomes a count of differing elements and the lowest of them.  A launch takes any number of pairs
// (a workgroup finds its pair by binary search over the pairs' first workgroups) and reports as the
// decoder's compare mode does: one atomicAdd and one atomicMin per workgroup that found a
// difference, none otherwise.
__global__ __launch_bounds__(256) void compare_kernel(const ComparePair* __restrict__ pairs, int n_pairs,
                                                      tk_wire_mismatch* report) {
  __shared__ uint32_t s_any[4];
  __shared__ unsigned long long s_red[8];
  int lo = 0, hi = n_pairs - 1;
  const int64_t blk = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pairs[mid].first_blk <= blk) lo = mid;
    else hi = mid - 1;
  }
  const ComparePair pr = pairs[lo];
  const int64_t at = ((blk - pr.first_blk) * 256 + threadIdx.x) * 16;
  uint32_t mask = 0;  // bit i: byte at + i differs
  if (at < pr.bytes) {
    const uint8_t* a = pr.expected + at;
    const uint8_t* b = pr.got + at;
    const uintptr_t both = (uintptr_t)a | (uintptr_t)b;
    if (at + 16 <= pr.bytes && (both & 3) == 0) {
      uint32_t x[4], y[4];
      if ((both & 15) == 0) {
        const tk_v4i p = __builtin_nontemporal_load(reinterpret_cast<const tk_v4i*>(a));
        const tk_v4i q = __builtin_nontemporal_load(reinterpret_cast<const tk_v4i*>(b));
        x[0] = (uint32_t)p.x, x[1] = (uint32_t)p.y, x[2] = (uint32_t)p.z, x[3] = (uint32_t)p.w;
        y[0] = (uint32_t)q.x, y[1] = (uint32_t)q.y, y[2] = (uint32_t)q.z, y[3] = (uint32_t)q.w;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          x[c] = reinterpret_cast<const uint32_t*>(a)[c], y[c] = reinterpret_cast<const uint32_t*>(b)[c];
      }
      if (x[0] != y[0] || x[1] != y[1] || x[2] != y[2] || x[3] != y[3]) {
#pragma unroll
        for (int j = 0; j < 16; ++j) mask |= (uint32_t)(wire_byte(x, j) != wire_byte(y, j)) << j;
      }
    } else {
      const int valid = (int)min((int64_t)16, pr.bytes - at);
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (j < valid) mask |= (uint32_t)(a[j] != b[j]) << j;
    }
  }
  uint32_t mis = 0;
  unsigned long long first = ~0ull;
  if (mask) {
    const int es = pr.elem_bytes;
    const uint32_t em = (1u << es) - 1u;
    for (int e = 16 / es - 1; e >= 0; --e)
      if ((mask >> (e * es)) & em) ++mis, first = (unsigned long long)(at / es + e);
  }
  wire_report_mismatches(mis, first, report + lo, s_any, s_red);
}

// pairs: device ComparePair[n_pairs] (first_blk filled, `blocks` their sum); report: device, n_pairs entries
static int compare_impl(const void* pairs, int n_pairs, int64_t blocks, tk_wire_mismatch* report, hipStream_t s) {
  TK_CHECK_ARG(pairs && report && n_pairs > 0 && blocks > 0 && blocks < ((int64_t)1 << 31), "bad arguments");
  hipLaunchKernelGGL(wire_report_init_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s, report, n_pairs);
  TK_LAUNCH_CHECK();
  hipLaunchKernelGGL(compare_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const ComparePair*)pairs, n_pairs, report);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// ---------------------------------------------------------------- digest
// Order-aware, parallel 64-bit digest: Σ_i mix(word_i ^ (i · φ)) mod 2^64 over
// little-endian 8-byte words (tail zero-padded).  Host twin: trace_format.digest_bytes.
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(kBlock) void digest_kernel(const uint8_t* __restrict__ p, int64_t nbytes,
                                                         unsigned long long* out) {
  int64_t nw = (nbytes + 7) / 8;
  int64_t stride = (int64_t)gridDim.x * kBlock;
  uint64_t acc = 0;
  for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < nw; i += stride) {
    uint64_t w = 0;
    if ((i + 1) * 8 <= nbytes) {
      __builtin_memcpy(&w, p + i * 8, 8);
    } else {
      for (int b = 0; i * 8 + b < nbytes; ++b) w |= (uint64_t)p[i * 8 + b] << (8 * b);
    }
    acc += mix64(w ^ ((uint64_t)i * 0x9E3779B97F4A7C15ULL));
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, (unsigned long long)acc);
}

}  // namespace tk

namespace {
// the encoders' view of a plan's segments: record i is read from src[i]
std::vector<tk::WireSegDev> source_segs(const tk::WirePlan& plan, const tk_wire_record* recs, const void* const* src,
                                        const tk_wire_addend* addends = nullptr) {
  std::vector<tk::WireSegDev> segs;
  segs.reserve(plan.segs.size());
  for (const tk::WireSegRef& r : plan.segs) {
    const int kind = tk::wire_seg_kind(recs[r.rec].kind);
    const tk::WireSegAddr a = tk::wire_seg_addr(r, kind, src[r.rec], recs[r.rec].diff ? src[r.rec - 1] : nullptr);
    segs.push_back({a.at, a.prev, r.n, kind, tk::wire_seg_bias(recs, addends, r.rec, r.e0)});
  }
  return segs;
}

// Device scratch kept between calls and only ever grown, because a trace job packs every chunk and
// hipFree would wait for the previous chunk's copy.  One call at a time uses it, holding `mu`.
struct DeviceScratch {
  std::mutex mu;
  void* dev = nullptr;
  int64_t bytes = 0;
  int device = -1;
  // *out: at least `need` bytes on the current device
  int reserve(int64_t need, char** out) {
    int cur = 0;
    TK_HIP(hipGetDevice(&cur));
    if (device != cur || bytes < need) {
      if (dev) (void)hipFree(dev);
      dev = nullptr, bytes = 0;
      TK_HIP(hipMalloc(&dev, (size_t)need));
      bytes = need, device = cur;
    }
    *out = (char*)dev;
    return TK_OK;
  }
};
// of tk_wire_pack_device: the segment list and the scan's levels
DeviceScratch g_pack_scratch;
// of tk_wire_unpack_device / tk_compare_device_batch: unit, segment or pair lists, the report and
// the status word
DeviceScratch g_unpack_scratch;
}  // namespace

extern "C" {

int tk_digest_bytes(const void* data, int64_t nbytes, uint64_t* out_device, void* stream) {
  hipStream_t s = tk::as_stream(stream);
  TK_CHECK_ARG(out_device && (data || nbytes == 0), "null argument");
  TK_HIP(hipMemsetAsync(out_device, 0, 8, s));
  if (nbytes == 0) return TK_OK;
  hipLaunchKernelGGL(tk::digest_kernel, dim3(tk::grid_for((nbytes + 7) / 8)), dim3(tk::kBlock), 0, s, (const uint8_t*)data,
                     nbytes, (unsigned long long*)out_device);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

int tk_wire_encode_device(const tk_wire_record* recs, int n_recs, const void* const* src, void* wire,
                          int64_t wire_cap, void* stream) {
  return tk_wire_encode_device_bias(recs, nullptr, n_recs, src, wire, wire_cap, stream);
}

int tk_wire_encode_device_bias(const tk_wire_record* recs, const tk_wire_addend* addends, int n_recs,
                               const void* const* src, void* wire, int64_t wire_cap, void* stream) {
  tk::WirePlan plan;
  if (const int rc = tk::wire_plan(recs, n_recs, -1, "tk_wire_encode_device", &plan, addends)) return rc;
  if (!src || !wire || wire_cap < plan.bound) {
    tk::set_error("tk_wire_encode_device: the wire buffer is smaller than tk_wire_bound");
    return TK_ERR_INVALID_ARG;
  }
  const std::vector<tk::WireSegDev> segs = source_segs(plan, recs, src, addends);
  hipStream_t s = tk::as_stream(stream);
  void* dev = nullptr;
  TK_HIP(hipMalloc(&dev, segs.size() * sizeof(tk::WireSegDev) + 64));
  uint32_t* cursor = (uint32_t*)((char*)dev + segs.size() * sizeof(tk::WireSegDev));
  int rc = TK_OK;
  if (hipMemcpyAsync(dev, segs.data(), segs.size() * sizeof(tk::WireSegDev), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemsetAsync(cursor, 0, sizeof(uint32_t), s) != hipSuccess) {
    tk::set_error("tk_wire_encode_device: loading the segment table failed");
    rc = TK_ERR_HIP;
  }
  if (rc == TK_OK) rc = tk::wire_encode_impl((const tk::WireSegDev*)dev, (int64_t)segs.size(), cursor, wire, plan.bound, s);
  if (hipStreamSynchronize(s) != hipSuccess && rc == TK_OK) {
    tk::set_error("tk_wire_encode_device: the encode kernel failed");
    rc = TK_ERR_HIP;
  }
  (void)hipFree(dev);
  return rc;
}

int64_t tk_wire_pack_device(const tk_wire_record* recs, int n_recs, const void* const* src, void* wire,
                            int64_t wire_cap, void* stream) {
  return tk_wire_pack_device_bias(recs, nullptr, n_recs, src, wire, wire_cap, stream);
}

int64_t tk_wire_pack_device_bias(const tk_wire_record* recs, const tk_wire_addend* addends, int n_recs,
                                 const void* const* src, void* wire, int64_t wire_cap, void* stream) {
  const char* who = addends ? "tk_wire_pack_device_bias" : "tk_wire_pack_device";  // errors name the entry point called
  tk::WirePlan plan;
  if (const int rc = tk::wire_plan(recs, n_recs, -1, who, &plan, addends)) return rc;
  if (!src || !wire || ((uintptr_t)wire & 63) != 0 || wire_cap < plan.bound) {
    tk::set_error(who, "the wire buffer is not 64-byte aligned or smaller than tk_wire_bound");
    return TK_ERR_INVALID_ARG;
  }
  const std::vector<tk::WireSegDev> segs = source_segs(plan, recs, src, addends);
  const int64_t n_seg = (int64_t)segs.size();
  const int64_t table = tk::wire_table_bytes(n_seg);
  const int64_t seg_bytes = tk::wire_align(n_seg * (int64_t)sizeof(tk::WireSegDev), 64);
  const int64_t words = tk::wire_scan_words(n_seg);
  hipStream_t s = tk::as_stream(stream);
  std::lock_guard<std::mutex> lock(g_pack_scratch.mu);
  char* dev = nullptr;
  int rc = g_pack_scratch.reserve(seg_bytes + 8 * words, &dev);
  if (rc != TK_OK) return rc;
  const tk::WireSegDev* dev_segs = (const tk::WireSegDev*)dev;
  uint64_t* scan = (uint64_t*)(dev + seg_bytes);
  TK_HIP(hipMemcpyAsync(dev, segs.data(), segs.size() * sizeof(tk::WireSegDev), hipMemcpyHostToDevice, s));
  rc = tk::wire_pack_plan_impl(dev_segs, n_seg, wire, scan, s);
  if (rc != TK_OK) return rc;
  uint64_t total = 0;  // payload units; the copy returns once the value is here
  TK_HIP(hipMemcpyAsync(&total, scan + words - 1, sizeof(total), hipMemcpyDeviceToHost, s));
  TK_HIP(hipStreamSynchronize(s));
  if (total > 0xFFFFFFF0ull) {
    tk::set_error(who, "the packed records do not fit the format's 32-bit segment starts");
    return TK_ERR_UNSUPPORTED;
  }
  const int64_t used = table + 64 * (int64_t)total;
  if (used > plan.bound) {
    tk::set_error(who, "the segment sizes exceed tk_wire_bound");
    return TK_ERR_HIP;
  }
  rc = tk::wire_pack_place_impl(dev_segs, n_seg, wire, used, s);
  if (rc != TK_OK) return rc;
  if (hipStreamSynchronize(s) != hipSuccess) {
    tk::set_error(who, "the place kernel failed");
    return TK_ERR_HIP;
  }
  return used;
}

int tk_wire_pack_tile(void) { return tk::kWireScanTile; }

int tk_wire_unpack_device(const tk_wire_record* recs, int n_recs, const void* wire, int64_t wire_bytes,
                          void* const* dst, int mode, tk_wire_mismatch* report, void* stream) {
  return tk_wire_unpack_device_bias(recs, nullptr, n_recs, wire, wire_bytes, dst, mode, report, stream);
}

int tk_wire_unpack_device_bias(const tk_wire_record* recs, const tk_wire_addend* addends, int n_recs, const void* wire,
                               int64_t wire_bytes, void* const* dst, int mode, tk_wire_mismatch* report,
                               void* stream) {
  const char* who = addends ? "tk_wire_unpack_device_bias" : "tk_wire_unpack_device";  // errors name the entry point called
  tk::WirePlan plan;
  if (const int rc = tk::wire_plan(recs, n_recs, -1, who, &plan, addends)) return rc;
  const bool compare = mode == TK_WIRE_UNPACK_COMPARE;
  if (!wire || !dst || ((uintptr_t)wire & 63) != 0 || (mode != TK_WIRE_UNPACK_STORE && !compare) ||
      (compare && !report)) {
    tk::set_error(who, "null argument, unknown mode or a wire buffer that is not 64-byte aligned");
    return TK_ERR_INVALID_ARG;
  }
  for (int i = 0; i < n_recs; ++i)
    if (tk::wire_seg_kind(recs[i].kind) == tk::kWireI32 && ((uintptr_t)dst[i] & 3) != 0) {
      tk::set_error(who, "the buffer of int32 record " + std::to_string(i) + " is not 4-byte aligned");
      return TK_ERR_INVALID_ARG;
    }
  const std::vector<tk::WireSegRef>& refs = plan.segs;
  const std::vector<tk::WireUnit>& units = plan.units;
  const int64_t n_seg = (int64_t)refs.size(), n_units = (int64_t)units.size();
  if (wire_bytes < tk::wire_table_bytes(n_seg)) {
    tk::set_error(who, "the segment table does not lie inside the wire buffer");
    return TK_ERR_INVALID_ARG;
  }
  std::vector<tk::WireSegOut> segs(refs.size());
  for (size_t i = 0; i < refs.size(); ++i)  // the decoder keeps the predecessor in registers: no prev
    segs[i] = {tk::wire_seg_addr(refs[i], recs[refs[i].rec].kind, dst[refs[i].rec], nullptr).at, refs[i].rec, 0};
  std::vector<tk::WireUnitDev> udev(units.size());
  for (size_t u = 0; u < units.size(); ++u) {
    const tk::WireSegRef& r = refs[units[u].first];
    udev[u] = {units[u].first, units[u].stride, units[u].count, r.n, tk::wire_seg_kind(recs[r.rec].kind), 0, r.e0};
  }
  // the bias table (and with it the instantiations that read one) only where a record has an addend
  std::vector<tk::WireBias> bias;
  for (size_t i = 0; i < refs.size(); ++i)
    if (tk::wire_addend_of(recs, addends, refs[i].rec)) {
      if (bias.empty()) bias.resize(refs.size());
      bias[i] = tk::wire_seg_bias(recs, addends, refs[i].rec, refs[i].e0);
    }
  const int64_t seg_bytes = tk::wire_align(n_seg * (int64_t)sizeof(tk::WireSegOut), 64);
  const int64_t unit_bytes = tk::wire_align(n_units * (int64_t)sizeof(tk::WireUnitDev), 64);
  const int64_t rep_bytes = tk::wire_align((int64_t)n_recs * (int64_t)sizeof(tk_wire_mismatch), 64);
  const int64_t bias_bytes = tk::wire_align((int64_t)bias.size() * (int64_t)sizeof(tk::WireBias), 64);
  hipStream_t s = tk::as_stream(stream);
  std::lock_guard<std::mutex> lock(g_unpack_scratch.mu);
  char* dev = nullptr;
  int rc = g_unpack_scratch.reserve(seg_bytes + unit_bytes + rep_bytes + 64 + bias_bytes, &dev);
  if (rc != TK_OK) return rc;
  char* dev_bias = bias.empty() ? nullptr : dev + seg_bytes + unit_bytes + rep_bytes + 64;
  if (dev_bias)
    TK_HIP(hipMemcpyAsync(dev_bias, bias.data(), bias.size() * sizeof(tk::WireBias), hipMemcpyHostToDevice, s));
  tk_wire_mismatch* rep = (tk_wire_mismatch*)(dev + seg_bytes + unit_bytes);
  uint32_t* status = (uint32_t*)(dev + seg_bytes + unit_bytes + rep_bytes);
  TK_HIP(hipMemcpyAsync(dev, segs.data(), segs.size() * sizeof(tk::WireSegOut), hipMemcpyHostToDevice, s));
  TK_HIP(hipMemcpyAsync(dev + seg_bytes, udev.data(), udev.size() * sizeof(tk::WireUnitDev), hipMemcpyHostToDevice, s));
  TK_HIP(hipMemsetAsync(status, 0, sizeof(uint32_t), s));
  rc = tk::wire_unpack_impl(dev + seg_bytes, n_units, dev, dev_bias, wire, n_seg, wire_bytes, mode, rep, n_recs, status, s);
  if (rc != TK_OK) return rc;
  uint32_t bad = 0;
  if (compare) TK_HIP(hipMemcpyAsync(report, rep, (size_t)n_recs * sizeof(tk_wire_mismatch), hipMemcpyDeviceToHost, s));
  TK_HIP(hipMemcpyAsync(&bad, status, sizeof(bad), hipMemcpyDeviceToHost, s));
  if (hipStreamSynchronize(s) != hipSuccess) {
    tk::set_error(who, "the decode kernel failed");
    return TK_ERR_HIP;
  }
  if (bad) {
    tk::set_error(who, "a segment does not lie inside the wire buffer or states a width its kind "
                  "does not have (was the buffer checked with tk_wire_check?)");
    return TK_ERR_INVALID_ARG;
  }
  return TK_OK;
}

int tk_compare_device_batch(const void* const* expected, const void* const* got, const int64_t* n_elems,
                            const int32_t* elem_bytes, int n, tk_wire_mismatch* report, void* stream) {
  if (!expected || !got || !n_elems || !elem_bytes || !report || n < 1) {
    tk::set_error("tk_compare_device_batch: null argument or no pairs");
    return TK_ERR_INVALID_ARG;
  }
  std::vector<tk::ComparePair> pairs;
  std::vector<int> index;  // pair of the launch -> pair of the call (empty pairs are not launched)
  int64_t blocks = 0;
  for (int i = 0; i < n; ++i) {
    const int es = elem_bytes[i];
    if ((es != 1 && es != 2 && es != 4 && es != 8) || n_elems[i] < 0 || n_elems[i] > ((int64_t)1 << 40) ||
        (n_elems[i] > 0 && (!expected[i] || !got[i]))) {
      tk::set_error("tk_compare_device_batch: pair " + std::to_string(i) +
                    " has a null buffer, a negative count or an element size other than 1, 2, 4, 8");
      return TK_ERR_INVALID_ARG;
    }
    report[i].mismatches = 0, report[i].first = ~(uint64_t)0;
    if (n_elems[i] == 0) continue;
    const int64_t bytes = n_elems[i] * es;
    pairs.push_back({(const uint8_t*)expected[i], (const uint8_t*)got[i], bytes, blocks, es, 0});
    index.push_back(i);
    blocks += (bytes + 4095) / 4096;
  }
  if (pairs.empty()) return TK_OK;
  if (blocks >= ((int64_t)1 << 31)) {
    tk::set_error("tk_compare_device_batch: too much to compare in one launch");
    return TK_ERR_UNSUPPORTED;
  }
  const int np = (int)pairs.size();
  const int64_t pair_bytes = tk::wire_align(np * (int64_t)sizeof(tk::ComparePair), 64);
  hipStream_t s = tk::as_stream(stream);
  std::lock_guard<std::mutex> lock(g_unpack_scratch.mu);
  char* dev = nullptr;
  int rc = g_unpack_scratch.reserve(pair_bytes + np * (int64_t)sizeof(tk_wire_mismatch), &dev);
  if (rc != TK_OK) return rc;
  tk_wire_mismatch* rep = (tk_wire_mismatch*)(dev + pair_bytes);
  TK_HIP(hipMemcpyAsync(dev, pairs.data(), pairs.size() * sizeof(tk::ComparePair), hipMemcpyHostToDevice, s));
  rc = tk::compare_impl(dev, np, blocks, rep, s);
  if (rc != TK_OK) return rc;
  std::vector<tk_wire_mismatch> out(np);
  TK_HIP(hipMemcpyAsync(out.data(), rep, (size_t)np * sizeof(tk_wire_mismatch), hipMemcpyDeviceToHost, s));
  if (hipStreamSynchronize(s) != hipSuccess) {
    tk::set_error("tk_compare_device_batch: the compare kernel failed");
    return TK_ERR_HIP;
  }
  for (int k = 0; k < np; ++k) report[index[k]] = out[k];
  return TK_OK;
}

int tk_compare_device(const void* expected, const void* got, int64_t n_elems, int elem_bytes,
                      tk_wire_mismatch* report, void* stream) {
  const int32_t es = elem_bytes;
  return tk_compare_device_batch(&expected, &got, &n_elems, &es, 1, report, stream);
}

}  // extern "C"
