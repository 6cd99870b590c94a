// Float statistics on the device, for gfx950: what relay.quantize's dataset calibration reduces the
// float32 records of a profile graph to -- value ranges, np.histogram's counts over given edges,
// and the digit counts of an exact radix select of |x| -- so that no activation leaves the device.
//
// The shape is tk_stats.hip's.  A plan owns a job table that is uploaded once; one launch takes
// every record of it.  A workgroup finds its record by binary search over the records' first
// workgroups and walks one span: kFStatsTiles tiles of kFStatsTile consecutive elements (a whole
// number of such spans where a record has more than kFStatsMaxGroups of them), a lane 16 bytes at a
// time with the next load in flight, every record byte read once per pass.  A buffer that is only
// 4-byte aligned is walked element by element, as is a record's ragged end.
//
// Three passes, each one launch:
//   range      count, the number of NaN / +-inf values, min and max of the finite ones.  Lanes keep
//              min / max as the order-preserving unsigned key of the float (sign set: ~bits, else
//              bits | 2^31); the flush turns the key back into the float and merges it with integer
//              atomics chosen by its sign (a non-negative float orders as a signed integer, a
//              negative one in reverse as an unsigned one).
//   histogram  np.histogram's rule over a record's own bins + 1 edges: x is counted in bin i when
//              edges[i] <= x < edges[i + 1], the last bin also takes x == edges[bins], anything
//              else (NaN included) is counted nowhere.  The bin is estimated in float32 and then
//              corrected against the edges (in LDS) by stepping down and up, so the edge array
//              alone defines the answer, as it does in numpy.  Counts are 32-bit LDS counters.
//   digits     one level of the radix select: the 31 magnitude bits split 11 + 10 + 10; an element
//              whose bits above the level's digit equal the record's prefix counts in its digit.
//
// Contention: post-ReLU records are about half exact zeros.  Zeros are counted in a register per
// lane and added to their bin once, at the flush; the digit pass also lets a lane whose four values
// share a digit issue one add of 4 (in the histogram pass, with 8001 bins, that test cost more than
// it saved and is compiled into profiling builds only).  A workgroup flushes once, with 64-bit atomic adds on the non-zero bins only: integer
// merges commute, so the result does not depend on arrival order.  No workgroup waits for another.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tk_fstats.h"

namespace tk {

static_assert(sizeof(tk_float_range) == 24, "tk_float_range has no padding");
static_assert(sizeof(FStatsJob) == 40, "FStatsJob has no padding");

int fstats_layout(const void* const* src, const int64_t* n_elems, int n, const char* who, std::vector<FStatsJob>* jobs,
                  int64_t* blocks) {
  const std::string w(who);
  if (!src || !n_elems || !jobs || !blocks || n <= 0) {
    set_error(w + ": null argument or no records");
    return TK_ERR_INVALID_ARG;
  }
  std::vector<FStatsJob> out;
  int64_t blk = 0;
  for (int i = 0; i < n; ++i) {
    if (n_elems[i] < 0 || n_elems[i] > ((int64_t)1 << 40) || (n_elems[i] > 0 && !src[i]) ||
        ((uintptr_t)src[i] & 3) != 0) {
      set_error(w + ": record " + std::to_string(i) +
                " has a null buffer, a bad element count or a buffer that is not 4-byte aligned");
      return TK_ERR_INVALID_ARG;
    }
    if (n_elems[i] == 0) continue;
    // all workgroups of a record flush into the same words: a record of more than kFStatsMaxGroups
    // spans is cut into that many longer ones instead (tk_stats.hip)
    const int64_t spans = (n_elems[i] + kFStatsSpan - 1) / kFStatsSpan;
    const int64_t span = (spans + kFStatsMaxGroups - 1) / kFStatsMaxGroups * kFStatsSpan;
    out.push_back({(const float*)src[i], n_elems[i], blk, span, i, 0});
    blk += (n_elems[i] + span - 1) / span;
  }
  if (blk >= ((int64_t)1 << 31)) {
    set_error(w + ": too many workgroups for one launch");
    return TK_ERR_INVALID_ARG;
  }
  *jobs = std::move(out);
  *blocks = blk;
  return TK_OK;
}

namespace {

typedef const __attribute__((address_space(1))) tk_v4i* FStatsLoad;  // record buffers are global memory

__device__ __forceinline__ FStatsJob fstats_job(const FStatsJob* __restrict__ jobs, int n_jobs, int64_t blk) {
  int lo = 0, hi = n_jobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].first_blk <= blk) lo = mid;
    else hi = mid - 1;
  }
  return jobs[lo];
}

// Walks elements [e0, e1) of a record as bit patterns: four(a, b, c, d) per 16-byte load, one(u) per
// element of the ragged end or of a buffer that is not 16-byte aligned.
template <class Four, class One>
__device__ __forceinline__ void fstats_walk(const float* __restrict__ src, int64_t e0, int64_t e1, Four four, One one) {
  const int tid = threadIdx.x;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(src);
  if (((uintptr_t)src & 15) != 0) {
    for (int64_t k = e0 + tid; k < e1; k += 256) one(p[k]);
    return;
  }
  int64_t e = e0 + (int64_t)tid * 4;  // spans start at multiples of 16 bytes
  bool have = e + 4 <= e1;
  tk_v4i next = {0, 0, 0, 0};
  if (have) next = __builtin_nontemporal_load((FStatsLoad)(p + e));
  while (have) {
    const tk_v4i v = next;
    e += 256 * 4;
    have = e + 4 <= e1;
    if (have) next = __builtin_nontemporal_load((FStatsLoad)(p + e));  // in flight while v is counted
    four((uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w);
  }
  for (int64_t k = e; k < e1; ++k) one(p[k]);  // the record's ragged end (one lane's)
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// ---------------------------------------------------------------- range

__device__ __forceinline__ uint32_t float_key(uint32_t u) { return (u >> 31) ? ~u : u | 0x80000000u; }
__device__ __forceinline__ uint32_t key_float(uint32_t k) { return (k >> 31) ? k & 0x7FFFFFFFu : ~k; }

__global__ __launch_bounds__(256) void fstats_range_kernel(const FStatsJob* __restrict__ jobs, int n_jobs,
                                                           tk_float_range* ranges) {
  __shared__ uint32_t s_mn[4], s_mx[4], s_bad[4];
  const int64_t blk = blockIdx.x;
  const FStatsJob job = fstats_job(jobs, n_jobs, blk);
  const int tid = threadIdx.x;
  const int64_t e0 = (blk - job.first_blk) * job.span;
  const int64_t e1 = min(job.n, e0 + job.span);
  // keys of finite values lie strictly between those of -inf and of the NaN 0x7FFFFFFF
  uint32_t mn = 0xFFFFFFFFu, mx = 0u, bad = 0u;
  auto one = [&](uint32_t u) {
    const bool finite = (u & 0x7F800000u) != 0x7F800000u;
    const uint32_t k = float_key(u);
    mn = min(mn, finite ? k : 0xFFFFFFFFu), mx = max(mx, finite ? k : 0u);
    bad += finite ? 0u : 1u;
  };
  fstats_walk(job.src, e0, e1, [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d) { one(a), one(b), one(c), one(d); },
              one);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    mn = min(mn, (uint32_t)__shfl_xor(mn, m, 64));
    mx = max(mx, (uint32_t)__shfl_xor(mx, m, 64));
  }
  bad = wave_sum(bad);
  if ((tid & 63) == 0) s_mn[tid >> 6] = mn, s_mx[tid >> 6] = mx, s_bad[tid >> 6] = bad;
  __syncthreads();
  tk_float_range* out = ranges + job.rec;
  if (tid == 0) {
    const uint32_t k = min(min(s_mn[0], s_mn[1]), min(s_mn[2], s_mn[3]));
    if (k != 0xFFFFFFFFu) {
      const uint32_t u = key_float(k);
      if (u >> 31) atomicMax(reinterpret_cast<unsigned int*>(&out->min), u);
      else atomicMin(reinterpret_cast<int*>(&out->min), (int)u);
    }
  }
  if (tid == 64) {
    const uint32_t k = max(max(s_mx[0], s_mx[1]), max(s_mx[2], s_mx[3]));
    if (k != 0u) {
      const uint32_t u = key_float(k);
      if (u >> 31) atomicMin(reinterpret_cast<unsigned int*>(&out->max), u);
      else atomicMax(reinterpret_cast<int*>(&out->max), (int)u);
    }
  }
  if (tid == 128) {
    atomicAdd(reinterpret_cast<unsigned long long*>(&out->count), (unsigned long long)(e1 - e0));
    const uint32_t b = s_bad[0] + s_bad[1] + s_bad[2] + s_bad[3];
    if (b) atomicAdd(reinterpret_cast<unsigned long long*>(&out->nonfinite), (unsigned long long)b);
  }
}

// The identity of the merge: no elements, min = +inf, max = -inf.
__global__ __launch_bounds__(256) void fstats_range_reset_kernel(unsigned long long* words, int64_t n_words) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_words) return;
  // word 2 holds min (low half) and max (high half)
  words[i] = i % 3 == 2 ? (0xFF800000ull << 32) | 0x7F800000ull : 0ull;
}

// ---------------------------------------------------------------- histogram over edges

// np.histogram's bin of x over `edges` (bins + 1 of them): -1 where x is counted nowhere.
__device__ __forceinline__ int fstats_bin(float x, const float* edges, int bins, float lo, float hi, float inv) {
  if (!(x >= lo && x <= hi)) return -1;           // NaN too
  const float t = (x - lo) * inv * (float)bins;  // an estimate only: the edges decide
  int i = (int)fminf(fmaxf(t, 0.0f), (float)(bins - 1));
  while (x < edges[i]) --i;  // x >= edges[0]
  while (i != bins - 1 && x >= edges[i + 1]) ++i;
  return i;
}

// kZeroReg: zeros are counted in a register and added at the flush; kLaneAdd: a lane whose four
// values share a bin issues one add of 4 (profiling builds only: it did not pay).
template <bool kZeroReg, bool kLaneAdd>
__global__ __launch_bounds__(256) void fstats_hist_kernel(const FStatsJob* __restrict__ jobs, int n_jobs,
                                                          const float* __restrict__ edges_all, int bins,
                                                          unsigned long long* hist_all) {
  __shared__ float s_edges[kFStatsMaxBins + 1];
  __shared__ uint32_t s_hist[kFStatsMaxBins];
  __shared__ uint32_t s_zero;
  const int64_t blk = blockIdx.x;
  const FStatsJob job = fstats_job(jobs, n_jobs, blk);
  const int tid = threadIdx.x;
  const float* edges = edges_all + (int64_t)job.rec * (bins + 1);
  for (int i = tid; i <= bins; i += 256) s_edges[i] = edges[i];
  for (int i = tid; i < bins; i += 256) s_hist[i] = 0;
  if (tid == 0) s_zero = 0;
  __syncthreads();
  const float lo = s_edges[0], hi = s_edges[bins];
  const float inv = 1.0f / (hi - lo);  // times bins: the estimate's scale, in two steps so that neither overflows
  const int64_t e0 = (blk - job.first_blk) * job.span;
  const int64_t e1 = min(job.n, e0 + job.span);
  uint32_t zeros = 0;
  // the bin of one value; -1 for a value counted nowhere and for a zero taken by the register
  auto bin = [&](uint32_t u) {
    if (kZeroReg && (u << 1) == 0u) {
      ++zeros;
      return -1;
    }
    return fstats_bin(__uint_as_float(u), s_edges, bins, lo, hi, inv);
  };
  auto one = [&](uint32_t u) {
    const int b = bin(u);
    if (b >= 0) atomicAdd(s_hist + b, 1u);
  };
  fstats_walk(
      job.src, e0, e1,
      [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
        const int s[4] = {bin(a), bin(b), bin(c), bin(d)};
        if (kLaneAdd && s[0] == s[1] && s[1] == s[2] && s[2] == s[3]) {
          if (s[0] >= 0) atomicAdd(s_hist + s[0], 4u);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (s[j] >= 0) atomicAdd(s_hist + s[j], 1u);
        }
      },
      one);
  if (kZeroReg) {
    zeros = wave_sum(zeros);
    if ((tid & 63) == 0 && zeros) atomicAdd(&s_zero, zeros);
  }
  __syncthreads();  // every count is in s_hist, every zero in s_zero
  if (kZeroReg && tid == 0 && s_zero) {
    const int b = fstats_bin(0.0f, s_edges, bins, lo, hi, inv);
    if (b >= 0) s_hist[b] += s_zero;
  }
  __syncthreads();
  unsigned long long* hist = hist_all + (int64_t)job.rec * bins;
  for (int i = tid; i < bins; i += 256) {
    const uint32_t c = s_hist[i];
    if (c) atomicAdd(hist + i, (unsigned long long)c);
  }
}

// ---------------------------------------------------------------- digits of |x|

__global__ __launch_bounds__(256) void fstats_digits_kernel(const FStatsJob* __restrict__ jobs, int n_jobs, int level,
                                                            const uint32_t* __restrict__ prefixes,
                                                            unsigned long long* hist_all) {
  __shared__ uint32_t s_hist[kFStatsDigits];
  __shared__ uint32_t s_zero;
  const int64_t blk = blockIdx.x;
  const FStatsJob job = fstats_job(jobs, n_jobs, blk);
  const int tid = threadIdx.x;
  const int used = level == 0 ? kFStatsDigits : 1024;
  for (int i = tid; i < used; i += 256) s_hist[i] = 0;
  if (tid == 0) s_zero = 0;
  __syncthreads();
  // level 0: digit = bits 30..20, no prefix; level 1: bits 19..10 under the 11 bits above them;
  // level 2: bits 9..0 under the 21 bits above them
  const int shift = level == 0 ? 20 : level == 1 ? 10 : 0;
  const uint32_t mask = level == 0 ? 2047u : 1023u;
  const int above = level == 0 ? 31 : level == 1 ? 20 : 10;
  const uint32_t prefix = level == 0 ? 0u : prefixes[job.rec];
  const int64_t e0 = (blk - job.first_blk) * job.span;
  const int64_t e1 = min(job.n, e0 + job.span);
  uint32_t zeros = 0;
  auto digit = [&](uint32_t u) {
    const uint32_t m = u & 0x7FFFFFFFu;  // |x|: -0.0 is 0
    if (m == 0u) {
      ++zeros;
      return -1;
    }
    if (level != 0 && (m >> above) != prefix) return -1;
    return (int)((m >> shift) & mask);
  };
  auto one = [&](uint32_t u) {
    const int b = digit(u);
    if (b >= 0) atomicAdd(s_hist + b, 1u);
  };
  fstats_walk(
      job.src, e0, e1,
      [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
        const int s[4] = {digit(a), digit(b), digit(c), digit(d)};
        if (s[0] == s[1] && s[1] == s[2] && s[2] == s[3]) {
          if (s[0] >= 0) atomicAdd(s_hist + s[0], 4u);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (s[j] >= 0) atomicAdd(s_hist + s[j], 1u);
        }
      },
      one);
  zeros = wave_sum(zeros);
  if ((tid & 63) == 0 && zeros) atomicAdd(&s_zero, zeros);
  __syncthreads();
  // a zero's digits are all 0: it counts at level 0, and below under the prefix 0
  if (tid == 0 && s_zero && prefix == 0u) s_hist[0] += s_zero;
  __syncthreads();
  unsigned long long* hist = hist_all + (int64_t)job.rec * kFStatsDigits;
  for (int i = tid; i < used; i += 256) {
    const uint32_t c = s_hist[i];
    if (c) atomicAdd(hist + i, (unsigned long long)c);
  }
}

// Which parts of the contention remedy the histogram pass uses: bit 0 zeros in registers, bit 1
// the whole-lane add.  Profiling builds (-DTK_ABLATION_BUILD) read TK_FSTATS_REMEDY; the product
// library always uses what the measurement kept: the zeros in registers.  The
// whole-lane add cost 5 % there, its four-way compare on every load for bins that rarely agree.
int fstats_remedy() {
#ifdef TK_ABLATION_BUILD
  const char* e = getenv("TK_FSTATS_REMEDY");
  if (e) return atoi(e) & 3;
#endif
  return 1;
}

}  // namespace
}  // namespace tk

struct tk_fstats_plan {
  tk::FStatsJob* jobs = nullptr;  // device
  int n_jobs = 0;                 // records of at least one element
  int n = 0;                      // entries of the result arrays
  int64_t blocks = 0;
};

extern "C" {

int tk_fstats_span(void) { return (int)tk::kFStatsSpan; }
int tk_float_range_size(void) { return (int)sizeof(tk_float_range); }

int tk_fstats_plan_create(const void* const* src, const int64_t* n_elems, int n, tk_fstats_plan** out) {
  if (!out) {
    tk::set_error("tk_fstats_plan_create: null argument");
    return TK_ERR_INVALID_ARG;
  }
  std::vector<tk::FStatsJob> jobs;
  int64_t blocks = 0;
  if (const int rc = tk::fstats_layout(src, n_elems, n, "tk_fstats_plan_create", &jobs, &blocks)) return rc;
  tk_fstats_plan* plan = new tk_fstats_plan();
  plan->n = n, plan->n_jobs = (int)jobs.size(), plan->blocks = blocks;
  if (!jobs.empty()) {
    const size_t bytes = jobs.size() * sizeof(tk::FStatsJob);
    if (hipMalloc((void**)&plan->jobs, bytes) != hipSuccess ||
        hipMemcpy(plan->jobs, jobs.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
      if (plan->jobs) (void)hipFree(plan->jobs);
      delete plan;
      tk::set_error("tk_fstats_plan_create: loading the job table failed");
      return TK_ERR_HIP;
    }
  }
  *out = plan;
  return TK_OK;
}

int tk_fstats_plan_destroy(tk_fstats_plan* plan) {
  if (!plan) return TK_OK;
  if (plan->jobs) (void)hipFree(plan->jobs);
  delete plan;
  return TK_OK;
}

int tk_float_range_reset(tk_float_range* ranges_dev, int n, void* stream) {
  TK_CHECK_ARG(ranges_dev && n > 0, "null argument or no entries");
  const int64_t words = (int64_t)n * 3;
  hipLaunchKernelGGL(tk::fstats_range_reset_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0,
                     tk::as_stream(stream), (unsigned long long*)ranges_dev, words);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

int tk_fstats_plan_range(tk_fstats_plan* plan, tk_float_range* ranges_dev, void* stream) {
  TK_CHECK_ARG(plan && ranges_dev, "null argument");
  if (plan->blocks == 0) return TK_OK;  // records of no elements only
  hipLaunchKernelGGL(tk::fstats_range_kernel, dim3((unsigned)plan->blocks), dim3(256), 0, tk::as_stream(stream),
                     (const tk::FStatsJob*)plan->jobs, plan->n_jobs, ranges_dev);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

int tk_fstats_plan_histogram(tk_fstats_plan* plan, const float* edges_dev, int bins, uint64_t* hist_dev, void* stream) {
  TK_CHECK_ARG(plan && edges_dev && hist_dev, "null argument");
  TK_CHECK_ARG(bins >= tk::kFStatsMinBins && bins <= tk::kFStatsMaxBins, "bins outside 2..8192");
  if (plan->blocks == 0) return TK_OK;
  const dim3 grid((unsigned)plan->blocks), block(256);
  hipStream_t s = tk::as_stream(stream);
  const tk::FStatsJob* jobs = plan->jobs;
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(hist_dev);
  switch (tk::fstats_remedy()) {
#ifdef TK_ABLATION_BUILD
    case 0: hipLaunchKernelGGL((tk::fstats_hist_kernel<false, false>), grid, block, 0, s, jobs, plan->n_jobs, edges_dev, bins, hist); break;
    case 2: hipLaunchKernelGGL((tk::fstats_hist_kernel<false, true>), grid, block, 0, s, jobs, plan->n_jobs, edges_dev, bins, hist); break;
    case 3: hipLaunchKernelGGL((tk::fstats_hist_kernel<true, true>), grid, block, 0, s, jobs, plan->n_jobs, edges_dev, bins, hist); break;
#endif
    default: hipLaunchKernelGGL((tk::fstats_hist_kernel<true, false>), grid, block, 0, s, jobs, plan->n_jobs, edges_dev, bins, hist); break;
  }
  TK_LAUNCH_CHECK();
  return TK_OK;
}

int tk_fstats_plan_digits(tk_fstats_plan* plan, int level, const uint32_t* prefix_dev, uint64_t* hist_dev,
                          void* stream) {
  TK_CHECK_ARG(plan && prefix_dev && hist_dev, "null argument");
  TK_CHECK_ARG(level >= 0 && level <= 2, "level outside 0..2");
  if (plan->blocks == 0) return TK_OK;
  hipLaunchKernelGGL(tk::fstats_digits_kernel, dim3((unsigned)plan->blocks), dim3(256), 0, tk::as_stream(stream),
                     (const tk::FStatsJob*)plan->jobs, plan->n_jobs, level, prefix_dev,
                     reinterpret_cast<unsigned long long*>(hist_dev));
  TK_LAUNCH_CHECK();
  return TK_OK;
}

}  // extern "C"

namespace tk {
namespace {

// The one-shot forms: device memory for `in_bytes` of arguments (uploaded from `in_host`, may be
// none) and `out_bytes` of results (`init` writes their identity), one pass, the copy out, one
// synchronisation.
template <class Init, class Run>
int fstats_one_shot(const char* who, const void* const* src, const int64_t* n_elems, int n, const void* in_host,
                    size_t in_bytes, void* out_host, size_t out_bytes, void* stream, Init init, Run run) {
  const std::string w(who);
  if (!out_host || (in_bytes && !in_host)) {
    set_error(w + ": null argument");
    return TK_ERR_INVALID_ARG;
  }
  tk_fstats_plan* plan = nullptr;
  if (const int rc = tk_fstats_plan_create(src, n_elems, n, &plan)) return rc;
  hipStream_t s = as_stream(stream);
  void *in_dev = nullptr, *out_dev = nullptr;
  int rc = TK_OK;
  if ((in_bytes && hipMalloc(&in_dev, in_bytes) != hipSuccess) || hipMalloc(&out_dev, out_bytes) != hipSuccess) {
    set_error(w + ": no device memory");
    rc = TK_ERR_HIP;
  }
  if (rc == TK_OK && in_bytes && hipMemcpyAsync(in_dev, in_host, in_bytes, hipMemcpyHostToDevice, s) != hipSuccess) {
    set_error(w + ": loading the arguments failed");
    rc = TK_ERR_HIP;
  }
  if (rc == TK_OK) rc = init(out_dev);
  if (rc == TK_OK) rc = run(plan, in_dev, out_dev);
  if (rc == TK_OK && hipMemcpyAsync(out_host, out_dev, out_bytes, hipMemcpyDeviceToHost, s) != hipSuccess) {
    set_error(w + ": reading the results failed");
    rc = TK_ERR_HIP;
  }
  if ((in_dev || out_dev) && hipStreamSynchronize(s) != hipSuccess && rc == TK_OK) {
    set_error(w + ": the kernel failed");
    rc = TK_ERR_HIP;
  }
  if (in_dev) (void)hipFree(in_dev);
  if (out_dev) (void)hipFree(out_dev);
  tk_fstats_plan_destroy(plan);
  return rc;
}

}  // namespace
}  // namespace tk

extern "C" {

int tk_float_range_batch(const void* const* src, const int64_t* n_elems, int n, tk_float_range* out_host,
                         void* stream) {
  const size_t bytes = (size_t)(n > 0 ? n : 0) * sizeof(tk_float_range);
  return tk::fstats_one_shot(
      "tk_float_range_batch", src, n_elems, n, nullptr, 0, out_host, bytes, stream,
      [&](void* out) { return tk_float_range_reset((tk_float_range*)out, n, stream); },
      [&](tk_fstats_plan* plan, void*, void* out) { return tk_fstats_plan_range(plan, (tk_float_range*)out, stream); });
}

int tk_float_histogram_batch(const void* const* src, const int64_t* n_elems, int n, const float* edges_host, int bins,
                             uint64_t* hist_host, void* stream) {
  if (bins < tk::kFStatsMinBins || bins > tk::kFStatsMaxBins) {
    tk::set_error("tk_float_histogram_batch: bins outside 2..8192");
    return TK_ERR_INVALID_ARG;
  }
  const size_t rows = (size_t)(n > 0 ? n : 0);
  return tk::fstats_one_shot(
      "tk_float_histogram_batch", src, n_elems, n, edges_host, rows * (bins + 1) * sizeof(float), hist_host,
      rows * bins * sizeof(uint64_t), stream,
      [&](void* out) {
        return hipMemsetAsync(out, 0, rows * bins * sizeof(uint64_t), tk::as_stream(stream)) == hipSuccess ? TK_OK
                                                                                                            : TK_ERR_HIP;
      },
      [&](tk_fstats_plan* plan, void* in, void* out) {
        return tk_fstats_plan_histogram(plan, (const float*)in, bins, (uint64_t*)out, stream);
      });
}

int tk_float_digits_batch(const void* const* src, const int64_t* n_elems, int n, int level, const uint32_t* prefix_host,
                          uint64_t* hist_host, void* stream) {
  if (level < 0 || level > 2) {
    tk::set_error("tk_float_digits_batch: level outside 0..2");
    return TK_ERR_INVALID_ARG;
  }
  const size_t rows = (size_t)(n > 0 ? n : 0);
  const size_t out_bytes = rows * tk::kFStatsDigits * sizeof(uint64_t);
  return tk::fstats_one_shot(
      "tk_float_digits_batch", src, n_elems, n, prefix_host, rows * sizeof(uint32_t), hist_host, out_bytes, stream,
      [&](void* out) { return hipMemsetAsync(out, 0, out_bytes, tk::as_stream(stream)) == hipSuccess ? TK_OK : TK_ERR_HIP; },
      [&](tk_fstats_plan* plan, void* in, void* out) {
        return tk_fstats_plan_digits(plan, level, (const uint32_t*)in, (uint64_t*)out, stream);
      });
}

}  // extern "C"
