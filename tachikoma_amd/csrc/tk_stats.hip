// Per-record statistics on the device, for gfx950: every record of a module reduced in one launch
// to exact integer statistics (tk_record_stats: count, sum, min, max, the histogram of magnitude
// bit lengths and, for 1-byte records, the histogram of values), merged into device-resident
// entries so that a dataset is calibrated without a record ever leaving the device.
//
// One launch takes every record of a job table.  A workgroup finds its record by binary search
// over the records' first workgroups and walks one span of it: kStatsTiles tiles of kStatsTile
// consecutive elements (a whole number of such spans where a record has more than kStatsMaxGroups
// of them), a lane 16 bytes at a time (one nontemporal 16-byte load: four int32 or
// sixteen 1-byte elements), every record byte read once.  Where the record's buffer is not 16-byte
// aligned the span is walked element by element, as is a span's ragged end.
//
// min, max and sum stay in registers and are reduced across the wave (shuffles), then across the
// workgroup (LDS).  The histograms are LDS counters, and the remedy for the contention of records
// that are mostly one value (post-ReLU zeros, clip bounds) is twofold: a lane whose 16 bytes are
// all equal (whose four int32 elements have one bit length) issues one add of 16 (4), and every
// bin is replicated -- 16 copies of the 256 value bins (copy = lane % 16, bin-major so that the copies of
// one bin lie in 16 different banks), 32 copies of the 33 bit-length bins of an int32 record -- so
// that at most 4 (2) lanes of a wave meet on one address.  A 1-byte record counts values only; its
// bit-length histogram is derived from the value bins when the workgroup flushes.
//
// A workgroup flushes once, after its span: one 32-bit atomicMin / atomicMax, 64-bit atomicAdds for
// count and sum, and one 64-bit atomicAdd per non-zero bin.  Integer merges commute, so the result
// does not depend on the order in which workgroups arrive and is equal on every run.  A span is
// 64 KiB of a 1-byte record and 256 KiB of an int32 record against at most 2.3 KiB (0.3 KiB) of
// flushed words.  No workgroup waits for another.
#include <climits>
#include <string>
#include <vector>

#include "tk_common.h"

namespace tk {

constexpr int kStatsTile = 4096;   // elements of one tile: 256 lanes x 16 bytes of a 1-byte record
constexpr int kStatsTiles = 16;    // tiles a workgroup walks before it flushes
constexpr int64_t kStatsSpan = (int64_t)kStatsTile * kStatsTiles;
constexpr int kStatsMaxGroups = 512;  // workgroups of one record: a larger record gets longer spans
constexpr int kStatsBits = 33, kStatsValues = 256;
constexpr int kValueCopies = 16, kBitCopies = 32;
constexpr int kStatsI32 = 0, kStatsI8 = 1, kStatsU8 = 2;

static_assert(sizeof(tk_record_stats) == 24 + 8 * (kStatsBits + kStatsValues), "tk_record_stats has no padding");

struct StatsJob {
  const uint8_t* src;
  int64_t n;          // elements, > 0
  int64_t first_blk;  // first workgroup of the record
  int64_t span;       // elements per workgroup: a whole number of kStatsSpan
  int32_t kind;
  int32_t rec;        // entry of the stats array
};

namespace {

struct LaneStats {
  int32_t mn, mx;
  unsigned long long sum;  // modulo 2^64
};

typedef unsigned short tk_v2us __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) tk_v4i* StatsLoad;  // record buffers are global memory

__device__ __forceinline__ int stats_bit_length(int32_t x) {
  const uint32_t ux = x < 0 ? 0u - (uint32_t)x : (uint32_t)x;
  return ux ? 32 - __builtin_clz(ux) : 0;
}

// An int32 record's span.  A lane's four elements take one LDS add where their bit lengths agree.
__device__ __forceinline__ void stats_span_i32(const uint8_t* __restrict__ src, int64_t e0, int64_t e1, uint32_t* hist,
                                               LaneStats& ls) {
  const int tid = threadIdx.x;
  const int copy = tid & (kBitCopies - 1);
  const int32_t* p = reinterpret_cast<const int32_t*>(src);
  auto one = [&](int32_t x) {
    ls.mn = min(ls.mn, x), ls.mx = max(ls.mx, x);
    ls.sum += (unsigned long long)(long long)x;
    atomicAdd(hist + stats_bit_length(x) * kBitCopies + copy, 1u);
  };
  if (((uintptr_t)src & 15) != 0) {
    for (int64_t k = e0 + tid; k < e1; k += 256) one(p[k]);
    return;
  }
  int64_t e = e0 + (int64_t)tid * 4;  // spans start at multiples of 16 bytes
  bool have = e + 4 <= e1;
  tk_v4i next = {0, 0, 0, 0};
  if (have) next = __builtin_nontemporal_load((StatsLoad)(p + e));
  while (have) {
    const tk_v4i v = next;
    e += 256 * 4;
    have = e + 4 <= e1;
    if (have) next = __builtin_nontemporal_load((StatsLoad)(p + e));  // in flight while v is counted
    const int32_t x[4] = {v.x, v.y, v.z, v.w};
    int slot[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ls.mn = min(ls.mn, x[j]), ls.mx = max(ls.mx, x[j]);
      ls.sum += (unsigned long long)(long long)x[j];
      slot[j] = stats_bit_length(x[j]) * kBitCopies + copy;
    }
    if (slot[0] == slot[1] && slot[1] == slot[2] && slot[2] == slot[3]) {
      atomicAdd(hist + slot[0], 4u);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(hist + slot[j], 1u);
    }
  }
  for (int64_t k = e; k < e1; ++k) one(p[k]);  // the record's ragged end (one lane's)
}

// A 1-byte record's span, in the biased domain u = v - dtype_min (the byte itself, or the byte with
// its sign bit flipped), which keeps the order: bin = u.  min / max are taken two 16-bit lanes at a
// time, the sum four bytes at a time; a lane's sixteen bytes take one LDS add where they are equal.
template <bool kSigned>
__device__ __forceinline__ void stats_span_8(const uint8_t* __restrict__ src, int64_t e0, int64_t e1, uint32_t* hist,
                                             LaneStats& ls) {
  constexpr uint32_t kFlip = kSigned ? 0x80808080u : 0u;
  const int tid = threadIdx.x;
  const int copy = tid & (kValueCopies - 1);
  tk_v2us mn2 = {0xFFFF, 0xFFFF}, mx2 = {0, 0};
  uint32_t usum = 0, cnt = 0;  // a lane sees span / 256 elements, at most 2^40 / kStatsMaxGroups / 256 = 2^23
  auto one = [&](uint32_t u) {
    mn2.x = min(mn2.x, (unsigned short)u), mx2.x = max(mx2.x, (unsigned short)u);
    usum += u, ++cnt;
    atomicAdd(hist + u * kValueCopies + copy, 1u);
  };
  if (((uintptr_t)src & 15) != 0) {
    for (int64_t k = e0 + tid; k < e1; k += 256) one(src[k] ^ (kFlip & 0xFFu));
  } else {
    int64_t e = e0 + (int64_t)tid * 16;  // spans start at multiples of 16 bytes
    bool have = e + 16 <= e1;
    tk_v4i next = {0, 0, 0, 0};
    if (have) next = __builtin_nontemporal_load((StatsLoad)(src + e));
    while (have) {
      const tk_v4i v = next;
      e += 256 * 16;
      have = e + 16 <= e1;
      if (have) next = __builtin_nontemporal_load((StatsLoad)(src + e));  // in flight while v is counted
      const uint32_t w[4] = {(uint32_t)v.x ^ kFlip, (uint32_t)v.y ^ kFlip, (uint32_t)v.z ^ kFlip, (uint32_t)v.w ^ kFlip};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t even = w[q] & 0x00FF00FFu, odd = (w[q] >> 8) & 0x00FF00FFu;
        tk_v2us a, b;
        __builtin_memcpy(&a, &even, 4);
        __builtin_memcpy(&b, &odd, 4);
        mn2 = __builtin_elementwise_min(mn2, __builtin_elementwise_min(a, b));
        mx2 = __builtin_elementwise_max(mx2, __builtin_elementwise_max(a, b));
        usum = __builtin_amdgcn_sad_u8(w[q], 0u, usum);
      }
      cnt += 16;
      if (w[0] == w[1] && w[1] == w[2] && w[2] == w[3] && w[0] == (w[0] & 0xFFu) * 0x01010101u) {
        atomicAdd(hist + (w[0] & 0xFFu) * kValueCopies + copy, 16u);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          atomicAdd(hist + ((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) * kValueCopies + copy, 1u);
      }
    }
    for (int64_t k = e; k < e1; ++k) one(src[k] ^ (kFlip & 0xFFu));  // the record's ragged end (one lane's)
  }
  if (cnt) {
    constexpr int32_t kBias = kSigned ? 128 : 0;
    ls.mn = (int32_t)min(mn2.x, mn2.y) - kBias, ls.mx = (int32_t)max(mx2.x, mx2.y) - kBias;
    ls.sum = (unsigned long long)((long long)usum - (long long)kBias * cnt);
  }
}

__global__ __launch_bounds__(256) void record_stats_kernel(const StatsJob* __restrict__ jobs, int n_jobs,
                                                           tk_record_stats* stats) {
  // value bins x 16 copies (1-byte kinds) or bit-length bins x 32 copies (int32), bin-major
  __shared__ uint32_t s_hist[kStatsValues * kValueCopies];
  __shared__ uint32_t s_bits[kStatsBits];
  __shared__ int32_t s_mn[4], s_mx[4];
  __shared__ unsigned long long s_sum[4];
  static_assert(kStatsBits * kBitCopies <= kStatsValues * kValueCopies, "the bit-length copies fit the value bins");
  int lo = 0, hi = n_jobs - 1;
  const int64_t blk = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].first_blk <= blk) lo = mid;
    else hi = mid - 1;
  }
  const StatsJob job = jobs[lo];
  const int tid = threadIdx.x;
  const int kind = job.kind;  // the same for the whole workgroup
  const int used = kind == kStatsI32 ? kStatsBits * kBitCopies : kStatsValues * kValueCopies;
  for (int i = tid; i < used; i += 256) s_hist[i] = 0;
  if (tid < kStatsBits) s_bits[tid] = 0;
  __syncthreads();
  const int64_t e0 = (blk - job.first_blk) * job.span;
  const int64_t e1 = min(job.n, e0 + job.span);
  LaneStats ls{INT32_MAX, INT32_MIN, 0ull};
  if (kind == kStatsI32) stats_span_i32(job.src, e0, e1, s_hist, ls);
  else if (kind == kStatsI8) stats_span_8<true>(job.src, e0, e1, s_hist, ls);
  else stats_span_8<false>(job.src, e0, e1, s_hist, ls);
  // min / max / sum: across the wave, then across the workgroup
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    ls.mn = min(ls.mn, __shfl_xor(ls.mn, m, 64));
    ls.mx = max(ls.mx, __shfl_xor(ls.mx, m, 64));
    ls.sum += __shfl_xor(ls.sum, m, 64);
  }
  if ((tid & 63) == 0) s_mn[tid >> 6] = ls.mn, s_mx[tid >> 6] = ls.mx, s_sum[tid >> 6] = ls.sum;
  __syncthreads();  // also: every count is in s_hist
  tk_record_stats* out = stats + job.rec;
  if (kind == kStatsI32) {
    if (tid < kStatsBits) {
      uint32_t c = 0;
#pragma unroll
      for (int k = 0; k < kBitCopies; ++k) c += s_hist[tid * kBitCopies + ((k + tid) & (kBitCopies - 1))];
      s_bits[tid] = c;
    }
  } else {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < kValueCopies; ++k) c += s_hist[tid * kValueCopies + ((k + tid) & (kValueCopies - 1))];
    if (c) {
      atomicAdd(reinterpret_cast<unsigned long long*>(&out->values[tid]), (unsigned long long)c);
      const int32_t v = kind == kStatsI8 ? tid - 128 : tid;
      atomicAdd(s_bits + stats_bit_length(v), c);
    }
  }
  __syncthreads();
  if (tid < kStatsBits && s_bits[tid])
    atomicAdd(reinterpret_cast<unsigned long long*>(&out->bits[tid]), (unsigned long long)s_bits[tid]);
  if (tid == 64) {
    atomicMin(&out->min, min(min(s_mn[0], s_mn[1]), min(s_mn[2], s_mn[3])));
    atomicMax(&out->max, max(max(s_mx[0], s_mx[1]), max(s_mx[2], s_mx[3])));
  }
  if (tid == 128) {
    atomicAdd(reinterpret_cast<unsigned long long*>(&out->count), (unsigned long long)(e1 - e0));
    atomicAdd(reinterpret_cast<unsigned long long*>(&out->sum), s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]);
  }
}

constexpr int kStatsWords = (int)(sizeof(tk_record_stats) / 8);

// The identity of the merge: no elements, min = INT32_MAX, max = INT32_MIN, empty histograms.
__global__ __launch_bounds__(256) void record_stats_reset_kernel(unsigned long long* words, int64_t n_words) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_words) return;
  // word 2 holds min (low half) and max (high half)
  words[i] = i % kStatsWords == 2 ? ((unsigned long long)(uint32_t)INT32_MIN << 32) | (uint32_t)INT32_MAX : 0ull;
}

}  // namespace
}  // namespace tk

struct tk_stats_plan {
  tk::StatsJob* jobs = nullptr;  // device
  int n_jobs = 0;                // records of at least one element
  int n = 0;                     // entries of the stats array
  int64_t blocks = 0;
};

extern "C" {

int tk_record_stats_tile(void) { return tk::kStatsTile; }
int tk_record_stats_span(void) { return (int)tk::kStatsSpan; }
int tk_record_stats_size(void) { return (int)sizeof(tk_record_stats); }

int tk_stats_plan_create(const void* const* src, const int64_t* n_elems, const int32_t* kinds, int n,
                         tk_stats_plan** out) {
  if (!src || !n_elems || !kinds || !out || n <= 0) {
    tk::set_error("tk_stats_plan_create: null argument or no records");
    return TK_ERR_INVALID_ARG;
  }
  std::vector<tk::StatsJob> jobs;
  int64_t blocks = 0;
  for (int i = 0; i < n; ++i) {
    if (kinds[i] < tk::kStatsI32 || kinds[i] > tk::kStatsU8) {
      tk::set_error("tk_stats_plan_create: record " + std::to_string(i) + " has kind " + std::to_string(kinds[i]) +
                    " (0 int32, 1 int8, 2 uint8 are supported)");
      return TK_ERR_UNSUPPORTED;
    }
    if (n_elems[i] < 0 || n_elems[i] > ((int64_t)1 << 40) || (n_elems[i] > 0 && !src[i]) ||
        (kinds[i] == tk::kStatsI32 && ((uintptr_t)src[i] & 3) != 0)) {
      tk::set_error("tk_stats_plan_create: record " + std::to_string(i) +
                    " has a null buffer, a bad element count or an int32 buffer that is not 4-byte aligned");
      return TK_ERR_INVALID_ARG;
    }
    if (n_elems[i] == 0) continue;
    // all workgroups of a record flush into one entry, and atomics on one address take their turns
    // (about 60 ns each): a record of more than kStatsMaxGroups spans is cut
    // into that many longer ones instead
    const int64_t spans = (n_elems[i] + tk::kStatsSpan - 1) / tk::kStatsSpan;
    const int64_t span = (spans + tk::kStatsMaxGroups - 1) / tk::kStatsMaxGroups * tk::kStatsSpan;
    jobs.push_back({(const uint8_t*)src[i], n_elems[i], blocks, span, kinds[i], i});
    blocks += (n_elems[i] + span - 1) / span;
  }
  if (blocks >= ((int64_t)1 << 31)) {
    tk::set_error("tk_stats_plan_create: too many workgroups for one launch");
    return TK_ERR_INVALID_ARG;
  }
  tk_stats_plan* plan = new tk_stats_plan();
  plan->n = n, plan->n_jobs = (int)jobs.size(), plan->blocks = blocks;
  if (!jobs.empty()) {
    const size_t bytes = jobs.size() * sizeof(tk::StatsJob);
    if (hipMalloc((void**)&plan->jobs, bytes) != hipSuccess ||
        hipMemcpy(plan->jobs, jobs.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
      if (plan->jobs) (void)hipFree(plan->jobs);
      delete plan;
      tk::set_error("tk_stats_plan_create: loading the job table failed");
      return TK_ERR_HIP;
    }
  }
  *out = plan;
  return TK_OK;
}

int tk_stats_plan_destroy(tk_stats_plan* plan) {
  if (!plan) return TK_OK;
  if (plan->jobs) (void)hipFree(plan->jobs);
  delete plan;
  return TK_OK;
}

int tk_record_stats_reset(tk_record_stats* stats_dev, int n, void* stream) {
  TK_CHECK_ARG(stats_dev && n > 0, "null argument or no entries");
  const int64_t words = (int64_t)n * tk::kStatsWords;
  hipLaunchKernelGGL(tk::record_stats_reset_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0,
                     tk::as_stream(stream), (unsigned long long*)stats_dev, words);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

int tk_stats_plan_run(tk_stats_plan* plan, tk_record_stats* stats_dev, void* stream) {
  TK_CHECK_ARG(plan && stats_dev, "null argument");
  if (plan->blocks == 0) return TK_OK;  // records of no elements only
  hipLaunchKernelGGL(tk::record_stats_kernel, dim3((unsigned)plan->blocks), dim3(256), 0, tk::as_stream(stream),
                     (const tk::StatsJob*)plan->jobs, plan->n_jobs, stats_dev);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

int tk_record_stats_batch(const void* const* src, const int64_t* n_elems, const int32_t* kinds, int n,
                          tk_record_stats* out_host, void* stream) {
  if (!out_host) {
    tk::set_error("tk_record_stats_batch: null argument");
    return TK_ERR_INVALID_ARG;
  }
  tk_stats_plan* plan = nullptr;
  if (const int rc = tk_stats_plan_create(src, n_elems, kinds, n, &plan)) return rc;
  hipStream_t s = tk::as_stream(stream);
  tk_record_stats* dev = nullptr;
  int rc = TK_OK;
  if (hipMalloc((void**)&dev, (size_t)n * sizeof(tk_record_stats)) != hipSuccess) {
    tk::set_error("tk_record_stats_batch: no device memory for the statistics");
    rc = TK_ERR_HIP;
  }
  if (rc == TK_OK) rc = tk_record_stats_reset(dev, n, stream);
  if (rc == TK_OK) rc = tk_stats_plan_run(plan, dev, stream);
  if (rc == TK_OK &&
      hipMemcpyAsync(out_host, dev, (size_t)n * sizeof(tk_record_stats), hipMemcpyDeviceToHost, s) != hipSuccess) {
    tk::set_error("tk_record_stats_batch: reading the statistics failed");
    rc = TK_ERR_HIP;
  }
  if (dev && hipStreamSynchronize(s) != hipSuccess && rc == TK_OK) {
    tk::set_error("tk_record_stats_batch: the statistics kernel failed");
    rc = TK_ERR_HIP;
  }
  if (dev) (void)hipFree(dev);
  tk_stats_plan_destroy(plan);
  return rc;
}

}  // extern "C"
