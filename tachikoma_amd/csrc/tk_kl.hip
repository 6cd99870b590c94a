// relay.quantize's kl_divergence threshold search (MinimizeKL, tk_calibrate.cc) on the device, for
// gfx950, over the histograms the float statistics leave there (tk_fstats.hip): every candidate
// window of every record is evaluated at once, and the few candidates that can be the host's
// argmin are listed for the host to confirm with its own code (tk_kl_candidates).
//
// The host's divergence is float32 arithmetic in a fixed sequential order, with a logf whose last
// place no device log reproduces.  So the device does not promise the host's value: it promises an
// interval that contains it.  Everything except the log and the final accumulation is done exactly
// as the host does it -- single IEEE float32 operations in the host's order, no contraction (the
// pragma below), hipcc's correctly rounded division, denormals kept: the tail folds into p[0] and
// p[len - 1], merged[j] / nz, both smooth steps, the sequential sums ps and qs, p / ps, q / qs and
// p / q.  p, q and the ratio are therefore the host's bits.  log and the running sum D are float64,
// and beside D runs a bound on |host's float32 partial sum - D| (tk_kl.h).
//
// evaluate  one lane per candidate, 256 consecutive candidates of one record per workgroup.  The
//           record's counts go to LDS once as int32 (32 KB; four workgroups fit a CU's 160 KB, so
//           the 61 waves of a default-size record and those of 60 more records are resident at
//           once).  Consecutive candidates start one bin apart, so a wave's LDS addresses are
//           consecutive.  A lane walks its window three times, bucket by bucket, each bucket after a
//           pre-pass for its sum and non-zero count: zero counts of p and q; the sums ps and qs; the
//           terms.  A bin with p == 0 has the same p, q and term throughout a candidate, so its log
//           is taken once.
// select    one workgroup per record: m = min(d + bound), then the candidates with d - bound <= m
//           in ascending order.
#include <cmath>
#include <limits>

#include "tk_kl.h"

#pragma clang fp contract(off)

namespace tk {
namespace {

static_assert(sizeof(tk_kl_row) == 32, "tk_kl_row has no padding");
static_assert(sizeof(tk_kl_pick) == 8 + 4 * TK_KL_MAX_PICKS, "tk_kl_pick has no padding");

// The window h[0 .. len) of one candidate, h[0] being bin lo of the record: calls
// f(p[t], q[t]) for t = 0 .. len - 1 with the host's p and q before smoothing.  win[0] is 0 on the
// host (bin lo is folded into p[0] with the left tail), so bucket 0 neither sums nor counts it.
template <class F>
__device__ __forceinline__ void kl_walk(const int32_t* h, int len, int per, int nq, float p0, float pl, F f) {
  for (int j = 0; j < nq; ++j) {
    const int a = j * per, b = j == nq - 1 ? len : a + per;
    uint32_t s = 0;  // the host's int sum, wrapping
    int nz = 0;
    for (int t = a; t < a + per; ++t) {
      const int32_t w = t ? h[t] : 0;
      s += (uint32_t)w, nz += w != 0;
    }
    float merged = (float)(int32_t)s;
    if (j == nq - 1) {  // the remainder bins fold into the last bucket: a second conversion and a float add
      uint32_t s2 = 0;
      for (int t = a + per; t < len; ++t) {
        const int32_t w = h[t];
        s2 += (uint32_t)w, nz += w != 0;
      }
      merged += (float)(int32_t)s2;
    }
    const float qv = nz ? merged / (float)nz : 0.f;
    for (int t = a; t < b; ++t) {
      const float pv = t == 0 ? p0 : t == len - 1 ? pl : (float)h[t];
      f(pv, pv != 0.f ? qv : 0.f);
    }
  }
}

__global__ __launch_bounds__(kKlLanes) void kl_evaluate_kernel(const unsigned long long* __restrict__ hist_all,
                                                               int num_bins, int nq, int n_cand, int groups,
                                                               tk_kl_row* __restrict__ table) {
  __shared__ int32_t s_h[kKlMaxBins];
  const int rec = blockIdx.x / groups, grp = blockIdx.x % groups;
  const int tid = threadIdx.x;
  const unsigned long long* hist = hist_all + (int64_t)rec * num_bins;
  int over = 0;
  for (int j = tid; j < num_bins; j += kKlLanes) {
    const unsigned long long c = hist[j];
    over |= c > 0x7FFFFFFFull;
    s_h[j] = (int32_t)(uint32_t)c;
  }
  over = __syncthreads_or(over);
  const int k = grp * kKlLanes + tid;
  if (k >= n_cand) return;  // no barrier below
  tk_kl_row* row = table + (int64_t)rec * n_cand + k;
  const double inf = std::numeric_limits<double>::infinity();
  if (over) {  // the select kernel reports it
    *row = tk_kl_row{inf, 0.0, 0.f, 0.f, 0, 0};
    return;
  }
  const int zero = num_bins / 2, i = nq / 2 + k;
  const int lo = zero - i, hi = zero + i + 1, len = hi - lo, per = len / nq;
  // the tails, in the host's j order: p[0] takes bins 0 .. lo, p[len - 1] bin hi - 1 and then hi .. end
  float p0 = 0.f;
  for (int j = 0; j <= lo; ++j) p0 += (float)s_h[j];
  float pl = (float)s_h[hi - 1];
  for (int j = hi; j < num_bins; ++j) pl += (float)s_h[j];
  const int32_t* h = s_h + lo;

  int zp = 0, zq = 0;
  kl_walk(h, len, per, nq, p0, pl, [&](float pv, float qv) { zp += pv == 0.f, zq += qv == 0.f; });
  // smooth(): empty if nothing is non-zero or the correction reaches 1
  const float eps1p = len - zp ? kKlEps * (float)zp / (float)(len - zp) : 0.f;
  const float eps1q = len - zq ? kKlEps * (float)zq / (float)(len - zq) : 0.f;
  const bool p_empty = len - zp == 0 || eps1p >= 1.0f, q_empty = len - zq == 0 || eps1q >= 1.0f;
  if (q_empty) {
    *row = tk_kl_row{inf, 0.0, 0.f, 0.f, zp, zq};
    return;
  }
  float ps = 0.f, qs = 0.f;
  kl_walk(h, len, per, nq, p0, pl, [&](float pv, float qv) {
    ps += pv == 0.f ? kKlEps : pv - eps1p;
    qs += qv == 0.f ? kKlEps : qv - eps1q;
  });
  if (p_empty) {  // the host's divergence() over an empty p: no term (not reachable below 10001 bins)
    *row = tk_kl_row{0.0, 0.0, 0.f, qs, zp, zq};
    return;
  }
  double D = 0.0, B = 0.0;
  bool unsure = false;  // a ratio outside the finite non-zero floats: no bound is claimed
  auto term = [&](float pn, float qn, double* t, double* tau) {
    const float r = pn / qn;
    if (!(r > 0.f) || r == std::numeric_limits<float>::infinity()) unsure = true;
    *t = (double)pn * log((double)r);
    *tau = kKlTermRel * fabs(*t) + kKlTermAbs;
  };
  auto add = [&](double t, double tau) {
    D += t;
    B = (B + tau) * (1.0 + kKlU) + kKlAddRel * fabs(D);
  };
  // a bin with p == 0 has q == 0 too: both become eps, the same term throughout the candidate
  const float pn0 = kKlEps / ps, qn0 = kKlEps / qs;
  const bool zero_counts = pn0 != 0.f && qn0 != 0.f;
  double t0 = 0.0, tau0 = 0.0;
  if (zp && zero_counts) term(pn0, qn0, &t0, &tau0);
  kl_walk(h, len, per, nq, p0, pl, [&](float pv, float qv) {
    if (pv == 0.f) {
      if (zero_counts) add(t0, tau0);
      return;
    }
    const float pn = (pv - eps1p) / ps;
    const float qn = (qv == 0.f ? kKlEps : qv - eps1q) / qs;
    if (pn != 0.f && qn != 0.f) {
      double t, tau;
      term(pn, qn, &t, &tau);
      add(t, tau);
    }
  });
  if (unsure || !(fabs(D) < inf)) D = 0.0, B = inf;  // survives every selection
  *row = tk_kl_row{D, B * kKlBoundSlack, ps, qs, zp, zq};
}

__global__ __launch_bounds__(256) void kl_select_kernel(const unsigned long long* __restrict__ hist_all, int num_bins,
                                                        int n_cand, const tk_kl_row* __restrict__ table,
                                                        tk_kl_pick* __restrict__ picks) {
  __shared__ double s_m[256];
  __shared__ int s_cnt[256];
  const int rec = blockIdx.x, tid = threadIdx.x;
  const unsigned long long* hist = hist_all + (int64_t)rec * num_bins;
  tk_kl_pick* pick = picks + rec;
  int over = 0;
  for (int j = tid; j < num_bins; j += 256) over |= hist[j] > 0x7FFFFFFFull;
  over = __syncthreads_or(over);
  if (tid < TK_KL_MAX_PICKS) pick->idx[tid] = -1;
  if (over) {
    if (tid == 0) pick->status = TK_KL_COUNT_OVERFLOW, pick->count = 0;
    return;
  }
  const tk_kl_row* rows = table + (int64_t)rec * n_cand;
  const int chunk = (n_cand + 255) / 256;  // a thread's consecutive candidates
  const int c0 = min(n_cand, tid * chunk), c1 = min(n_cand, c0 + chunk);
  const double inf = std::numeric_limits<double>::infinity();
  double m = inf;
  for (int c = c0; c < c1; ++c) m = fmin(m, rows[c].d + rows[c].bound);
  s_m[tid] = m;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) s_m[tid] = fmin(s_m[tid], s_m[tid + w]);
    __syncthreads();
  }
  m = s_m[0];
  if (m == inf) {  // the same for every thread
    if (tid == 0) pick->status = TK_KL_ALL_INF, pick->count = 0;
    return;
  }
  int cnt = 0;
  for (int c = c0; c < c1; ++c) cnt += rows[c].d - rows[c].bound <= m;
  s_cnt[tid] = cnt;
  __syncthreads();  // also orders the idx reset above before the writes below
  int at = 0;
  for (int t = 0; t < tid; ++t) at += s_cnt[t];
  for (int c = c0; c < c1; ++c)
    if (rows[c].d - rows[c].bound <= m) {
      if (at < TK_KL_MAX_PICKS) pick->idx[at] = c;
      ++at;
    }
  if (tid == 255) pick->count = at, pick->status = at > TK_KL_MAX_PICKS ? TK_KL_TOO_MANY : TK_KL_OK;
}

int kl_check(const char* who, const void* hist_dev, int n, int num_bins, int nq, const void* a, const void* b) {
  if (!hist_dev || !a || !b || n <= 0) {
    set_error(std::string(who) + ": null argument or no records");
    return TK_ERR_INVALID_ARG;
  }
  if (num_bins < 3 || num_bins >= kKlMaxBins || num_bins % 2 == 0 || nq < 2 || nq > num_bins) {
    set_error(std::string(who) + ": num_bins must be odd in 3..8191 and num_quantized_bins lie in 2..num_bins");
    return TK_ERR_INVALID_ARG;
  }
  return TK_OK;
}

}  // namespace
}  // namespace tk

extern "C" {

int tk_kl_row_size(void) { return (int)sizeof(tk_kl_row); }
int tk_kl_pick_size(void) { return (int)sizeof(tk_kl_pick); }

int tk_kl_device_evaluate(const uint64_t* hist_dev, int n, int num_bins, int num_quantized_bins, tk_kl_row* table_dev,
                          void* stream) {
  if (const int rc = tk::kl_check("tk_kl_device_evaluate", hist_dev, n, num_bins, num_quantized_bins, table_dev, table_dev))
    return rc;
  const int n_cand = num_bins / 2 + 1 - num_quantized_bins / 2;
  const int groups = (n_cand + tk::kKlLanes - 1) / tk::kKlLanes;
  TK_CHECK_ARG((int64_t)n * groups < ((int64_t)1 << 31), "too many workgroups for one launch");
  hipLaunchKernelGGL(tk::kl_evaluate_kernel, dim3((unsigned)(n * groups)), dim3(tk::kKlLanes), 0, tk::as_stream(stream),
                     reinterpret_cast<const unsigned long long*>(hist_dev), num_bins, num_quantized_bins, n_cand, groups,
                     table_dev);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

int tk_kl_device_select(const uint64_t* hist_dev, int n, int num_bins, int num_quantized_bins,
                        const tk_kl_row* table_dev, tk_kl_pick* picks_dev, void* stream) {
  if (const int rc = tk::kl_check("tk_kl_device_select", hist_dev, n, num_bins, num_quantized_bins, table_dev, picks_dev))
    return rc;
  const int n_cand = num_bins / 2 + 1 - num_quantized_bins / 2;
  hipLaunchKernelGGL(tk::kl_select_kernel, dim3((unsigned)n), dim3(256), 0, tk::as_stream(stream),
                     reinterpret_cast<const unsigned long long*>(hist_dev), num_bins, n_cand, table_dev, picks_dev);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

int tk_kl_device(const uint64_t* hist_dev, int n, int num_bins, int num_quantized_bins, tk_kl_row* table_dev,
                 tk_kl_pick* picks_dev, void* stream) {
  if (const int rc = tk::kl_check("tk_kl_device", hist_dev, n, num_bins, num_quantized_bins, table_dev, picks_dev))
    return rc;
  if (const int rc = tk_kl_device_evaluate(hist_dev, n, num_bins, num_quantized_bins, table_dev, stream)) return rc;
  return tk_kl_device_select(hist_dev, n, num_bins, num_quantized_bins, table_dev, picks_dev, stream);
}

}  // extern "C"
