// Batched shadow rebuild: the int8 shadows ([C_pad16/16][N*HW][16], tk_conv2d_make_shadow layout)
// of many NCHW 8-bit tensors in one launch, for a module whose record buffers were loaded from a
// trace file (GraphModule.replay_trace / load_trace(shadows=True)).
//
// Work item = (tensor, image, 16-channel chunk, tile of kTilePix pixels), one wave per item.  The
// 64 lanes are four 16-lane groups; in each step a group takes 16 consecutive pixels, lane l of it
// loading channel l's 16 bytes (one 16-byte load, four 4-byte loads or bytes, as the plane's
// address allows) and writing them as row l of the group's 16x16 LDS tile; after the barrier lane l
// gathers column l (pixel l's 16 channels) and stores it as one 16-byte store, contiguous across
// the wave.  The item list is laid out on the host once per list of tensors and kept on the device
// (ShadowTables below), as a module rebuilds the same shadows for every file it replays.
#include <algorithm>
#include <list>
#include <mutex>
#include <vector>

#include "tk_common.h"
#include "tk_conv.h"

namespace tk {

struct ShadowTensor {
  const uint8_t* src;
  uint8_t* dst;
  int32_t N, C, HW;
  int32_t flip;  // uint8 data: stored xor 0x80
  bool operator==(const ShadowTensor& o) const {
    return src == o.src && dst == o.dst && N == o.N && C == o.C && HW == o.HW && flip == o.flip;
  }
};
struct ShadowItem {
  int32_t tensor, n, chunk, pix0;
};
static_assert(sizeof(ShadowTensor) == 32 && sizeof(ShadowItem) == 16, "device table layout");

constexpr int kShadowWaves = 4;                  // items per workgroup
constexpr int kShadowSteps = 4;                  // 64 pixels each
constexpr int kTilePix = 64 * kShadowSteps;      // pixels of an item
// a group's tile: 16 rows of 16 bytes, plus one row of padding so that the four groups of a wave
// (and the two of a 32-lane half) read different banks when they gather the same column
constexpr int kGroupBytes = 16 * 16 + 16;

__global__ __launch_bounds__(64 * kShadowWaves) void shadow_batch_kernel(const ShadowTensor* __restrict__ tensors,
                                                                         const ShadowItem* __restrict__ items,
                                                                         int64_t n_items) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kShadowWaves * 4 * kGroupBytes];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, l = lane & 15;
  const int64_t it = (int64_t)blockIdx.x * kShadowWaves + wave;
  const bool live = it < n_items;  // (a dead wave of the last workgroup only keeps the barriers)
  const ShadowItem item = items[live ? it : 0];
  const ShadowTensor t = tensors[item.tensor];
  uint8_t* tile = lds + (wave * 4 + g) * kGroupBytes;
  const int c = item.chunk * 16 + l;
  const bool real = c < t.C;  // else a padded channel: zeros, nothing is read
  const uint8_t* plane = t.src + ((int64_t)item.n * t.C + (real ? c : 0)) * t.HW;
  uint8_t* out = t.dst + ((int64_t)item.chunk * t.N + item.n) * t.HW * 16;
  const uint32_t flip = t.flip ? 0x80808080u : 0u;
  for (int step = 0; step < kShadowSteps; ++step) {
    const int p0 = item.pix0 + step * 64;
    const bool active = live && p0 < t.HW;  // the same in every lane of the wave
    if (active) {
      const int gp = p0 + g * 16;  // the group's first pixel
      uint32_t v[4] = {0u, 0u, 0u, 0u};
      if (real && gp < t.HW) {
        const uint8_t* a = plane + gp;
        if (gp + 16 <= t.HW && ((uintptr_t)a & 15) == 0) {
          const tk_v4i w = ldg(reinterpret_cast<const tk_v4i*>(a));
          v[0] = (uint32_t)w.x, v[1] = (uint32_t)w.y, v[2] = (uint32_t)w.z, v[3] = (uint32_t)w.w;
        } else if (gp + 16 <= t.HW && ((uintptr_t)a & 3) == 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = ldg(reinterpret_cast<const uint32_t*>(a + 4 * q));
        } else {
          // an unaligned plane, or the last pixels of one: element by element
          const int m = min(16, t.HW - gp);
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if (j < m) v[j >> 2] |= (uint32_t)ldg(a + j) << (8 * (j & 3));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] ^= flip;
      }
      *reinterpret_cast<uint4*>(tile + l * 16) = make_uint4(v[0], v[1], v[2], v[3]);
    }
    lds_barrier();
    if (active) {
      const int p = p0 + g * 16 + l;
      if (p < t.HW) {
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          o[k] = (uint32_t)tile[(4 * k) * 16 + l] | ((uint32_t)tile[(4 * k + 1) * 16 + l] << 8) |
                 ((uint32_t)tile[(4 * k + 2) * 16 + l] << 16) | ((uint32_t)tile[(4 * k + 3) * 16 + l] << 24);
        const tk_v4i w = {(int)o[0], (int)o[1], (int)o[2], (int)o[3]};
        *(__attribute__((address_space(1))) tk_v4i*)(out + (int64_t)p * 16) = w;
      }
    }
    lds_barrier();  // the tile is rewritten in the next step (the stores stay in flight)
  }
}

namespace {

// The device tables of the lists of tensors seen so far: the tensor and item tables are a function
// of the list alone (addresses, shapes, dtypes), so a module that rebuilds its shadows for every
// file lays them out and uploads them once.  A few lists are kept (one per live module, in
// practice); the oldest is freed when another arrives, which waits for the device (hipFree) and
// so cannot pull the table from under a launch that still reads it.
struct ShadowTable {
  int device = -1;
  std::vector<ShadowTensor> key;
  std::vector<char> host;  // what was uploaded (the copy's source stays alive with the entry)
  char* dev = nullptr;
  int64_t n_items = 0;
  hipEvent_t uploaded = nullptr;  // a launch on another stream waits for the upload
};
struct ShadowTables {
  std::mutex mu;
  std::list<ShadowTable> entries;  // most recently used first
  static constexpr size_t kKeep = 8;
};
ShadowTables g_shadow_tables;

void release(ShadowTable& e) {
  if (e.dev) (void)hipFree(e.dev);
  if (e.uploaded) (void)hipEventDestroy(e.uploaded);
  e.dev = nullptr, e.uploaded = nullptr;
}

int64_t lay_out(const std::vector<ShadowTensor>& key, std::vector<char>* host) {
  std::vector<ShadowItem> items;
  for (size_t i = 0; i < key.size(); ++i) {
    const ShadowTensor& t = key[i];
    const int chunks = (t.C + 15) / 16;
    // in the order of the shadow's memory: consecutive items write consecutive bytes
    for (int chunk = 0; chunk < chunks; ++chunk)
      for (int n = 0; n < t.N; ++n)
        for (int p = 0; p < t.HW; p += kTilePix) items.push_back({(int32_t)i, n, chunk, p});
  }
  const size_t tb = key.size() * sizeof(ShadowTensor), ib = items.size() * sizeof(ShadowItem);
  host->resize(tb + ib);
  if (tb) __builtin_memcpy(host->data(), key.data(), tb);
  if (ib) __builtin_memcpy(host->data() + tb, items.data(), ib);
  return (int64_t)items.size();
}

}  // namespace

int make_shadow_batch_impl(const tk_tensor* const* data, void* const* shadow, int n, hipStream_t s) {
  TK_CHECK_ARG(n >= 0, "negative count");
  if (n == 0) return TK_OK;
  TK_CHECK_ARG(data && shadow, "null argument");
  std::vector<ShadowTensor> key;
  key.reserve(n);
  int64_t n_items = 0;
  for (int i = 0; i < n; ++i) {
    const tk_tensor* t = data[i];
    TK_CHECK_ARG(t && shadow[i] && t->data, "tensor " + std::to_string(i) + ": null tensor or shadow");
    TK_CHECK_ARG(t->ndim == 4 && is_int8ish(t) && compact(t),
                 "tensor " + std::to_string(i) + " must be a compact 4-D int8/uint8 tensor");
    TK_CHECK_ARG(((uintptr_t)shadow[i] & 15) == 0, "shadow " + std::to_string(i) + " is not 16-byte aligned");
    const int64_t N = t->shape[0], C = t->shape[1], HW = t->shape[2] * t->shape[3];
    TK_CHECK_ARG(N >= 0 && C >= 0 && t->shape[2] >= 0 && t->shape[3] >= 0 && N < (1 << 30) && C < (1 << 30) &&
                     HW < (1 << 30),
                 "tensor " + std::to_string(i) + ": extent out of range");
    if (N == 0 || C == 0 || HW == 0) continue;  // nothing to write
    key.push_back({(const uint8_t*)ptr(t), (uint8_t*)shadow[i], (int32_t)N, (int32_t)C, (int32_t)HW,
                   (int32_t)is_uint(t, 8)});
    n_items += ((C + 15) / 16) * N * ((HW + kTilePix - 1) / kTilePix);
  }
  if (key.empty()) return TK_OK;
  if ((n_items + kShadowWaves - 1) / kShadowWaves >= ((int64_t)1 << 31)) {
    set_error("tk_conv2d_make_shadow_batch: too many work items for one launch");
    return TK_ERR_UNSUPPORTED;
  }
  int cur = 0;
  TK_HIP(hipGetDevice(&cur));
  std::lock_guard<std::mutex> lock(g_shadow_tables.mu);
  auto& entries = g_shadow_tables.entries;
  auto hit = std::find_if(entries.begin(), entries.end(),
                          [&](const ShadowTable& e) { return e.device == cur && e.key == key; });
  if (hit != entries.end()) {
    entries.splice(entries.begin(), entries, hit);
  } else {
    while (entries.size() >= ShadowTables::kKeep) {
      release(entries.back());
      entries.pop_back();
    }
    ShadowTable e;
    e.device = cur;
    e.n_items = lay_out(key, &e.host);
    e.key = std::move(key);
    entries.push_front(std::move(e));
    ShadowTable& f = entries.front();
    hipError_t rc = hipMalloc((void**)&f.dev, f.host.size());
    if (rc == hipSuccess) rc = hipEventCreateWithFlags(&f.uploaded, hipEventDisableTiming);
    if (rc == hipSuccess) rc = hipMemcpyAsync(f.dev, f.host.data(), f.host.size(), hipMemcpyHostToDevice, s);
    if (rc == hipSuccess) rc = hipEventRecord(f.uploaded, s);
    if (rc != hipSuccess) {
      set_error(std::string("tk_conv2d_make_shadow_batch: loading the item table failed: ") + hipGetErrorString(rc));
      release(f);
      entries.pop_front();
      return TK_ERR_HIP;
    }
  }
  const ShadowTable& e = entries.front();
  TK_HIP(hipStreamWaitEvent(s, e.uploaded, 0));
  const int64_t blocks = (e.n_items + kShadowWaves - 1) / kShadowWaves;
  hipLaunchKernelGGL(shadow_batch_kernel, dim3((unsigned)blocks), dim3(64 * kShadowWaves), 0, s,
                     (const ShadowTensor*)e.dev, (const ShadowItem*)(e.dev + e.key.size() * sizeof(ShadowTensor)),
                     e.n_items);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

}  // namespace tk

extern "C" {

int tk_conv2d_make_shadow_batch(const tk_tensor* const* data, void* const* shadow, int n, void* stream) {
  return tk::make_shadow_batch_impl(data, shadow, n, tk::as_stream(stream));
}

}  // extern "C"
