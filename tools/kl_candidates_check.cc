// Stand-alone check of tk_kl_candidates (csrc/tk_calibrate.cc) for sanitizer builds: a candidate
// list in any order -- reversed, strided, with repeats -- gives rows equal to those of a full run,
// the first minimum of the full run is the window tk_find_scale_by_kl returns, and every refusal
// leaves the output alone.  CPU only; never needs a device.
//
//   hipcc -std=c++20 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=all -I include tools/kl_candidates_check.cc \
//       -x hip tachikoma_amd/csrc/tk_calibrate.cc -o kl_candidates_check && ./kl_candidates_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../tachikoma_amd/csrc/tk_common.h"

namespace tk {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace tk

static int g_fail = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);     \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

static bool same(const tk_kl_candidate& a, const tk_kl_candidate& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static void check_shape(int bins, int buckets, int kind) {
  std::vector<int32_t> hist(bins, 0);
  uint32_t x = 12345u + (uint32_t)kind;
  for (int j = 0; j < bins; ++j) {
    x = x * 1664525u + 1013904223u;
    const int d = j - bins / 2;
    int32_t c = (int32_t)((x >> 16) % 1000u) * (d * d < bins * bins / 16 ? 20 : 1);
    if (kind == 1 && d < 0) c = 0;                                // post-ReLU
    if (kind == 2 && j % 50 != (bins / 2) % 50) c = 0;            // sparse
    if (kind == 3) c = (j < 2 || j >= bins - 2) ? c + 1 : 0;      // extremes: narrow windows are +inf
    if (kind == 4) c = j == 0 || j == bins - 1 ? (1 << 24) + 1 + c : c;  // the folds round
    hist[j] = c;
  }
  std::vector<float> edges(bins + 1);
  for (int j = 0; j <= bins; ++j) edges[j] = -2.f + 4.f * (float)j / (float)bins;
  const int n = bins / 2 + 1 - buckets / 2;
  std::vector<int32_t> all(n);
  for (int k = 0; k < n; ++k) all[k] = k;
  std::vector<tk_kl_candidate> full(n);
  CHECK(tk_kl_candidates(hist.data(), bins, buckets, all.data(), n, full.data()) == TK_OK);
  int best = 0;
  for (int k = 1; k < n; ++k)
    if (full[k].div < full[best].div) best = k;
  float thr = 0.f;
  CHECK(tk_find_scale_by_kl(hist.data(), edges.data(), bins, buckets, &thr) == TK_OK);
  CHECK(thr == edges[bins / 2 + buckets / 2 + best + 1]);
  // reversed, strided and repeated lists
  std::vector<int32_t> list;
  for (int k = n - 1; k >= 0; --k) list.push_back(k);
  for (int k = 0; k < n; k += 3) list.push_back(k), list.push_back(k);
  std::vector<tk_kl_candidate> got(list.size());
  CHECK(tk_kl_candidates(hist.data(), bins, buckets, list.data(), (int)list.size(), got.data()) == TK_OK);
  for (size_t c = 0; c < list.size(); ++c) CHECK(same(got[c], full[list[c]]));
  CHECK(tk_kl_candidates(hist.data(), bins, buckets, list.data(), 0, got.data()) == TK_OK);
}

int main() {
  CHECK(tk_kl_candidate_size() == (int)sizeof(tk_kl_candidate) && sizeof(tk_kl_candidate) == 20);
  const int shapes[6][2] = {{3, 2}, {11, 3}, {101, 11}, {255, 255}, {257, 255}, {1023, 2}};
  for (const auto& s : shapes)
    for (int kind = 0; kind < 5; ++kind) check_shape(s[0], s[1], kind);
  check_shape(8001, 255, 1);

  // refusals write nothing
  std::vector<int32_t> hist(102, 1);
  int32_t cand[2] = {0, 1};
  tk_kl_candidate out[2];
  std::memset(out, 0x5A, sizeof out);
  tk_kl_candidate untouched[2];
  std::memcpy(untouched, out, sizeof out);
  auto refused = [&](const int32_t* h, int bins, int buckets, const int32_t* c, int n, tk_kl_candidate* o) {
    tk::g_err.clear();
    CHECK(tk_kl_candidates(h, bins, buckets, c, n, o) == TK_ERR_INVALID_ARG);
    CHECK(tk::g_err.rfind("tk_kl_candidates: ", 0) == 0);
    CHECK(std::memcmp(out, untouched, sizeof out) == 0);
  };
  refused(nullptr, 101, 11, cand, 2, out);
  refused(hist.data(), 101, 11, nullptr, 2, out);
  refused(hist.data(), 101, 11, cand, 2, nullptr);
  refused(hist.data(), 100, 11, cand, 2, out);  // even
  refused(hist.data(), 102, 11, cand, 2, out);
  refused(hist.data(), 1, 2, cand, 2, out);
  refused(hist.data(), 101, 1, cand, 2, out);
  refused(hist.data(), 101, 102, cand, 2, out);
  refused(hist.data(), 101, 11, cand, -1, out);
  const int32_t past[2] = {0, 46};  // 101 / 2 + 1 - 11 / 2 = 46 candidates: 0..45
  refused(hist.data(), 101, 11, past, 2, out);
  const int32_t negative[2] = {-1, 0};
  refused(hist.data(), 101, 11, negative, 2, out);
  std::printf(g_fail ? "kl_candidates_check: %d failures\n" : "kl_candidates_check: ok\n", g_fail);
  return g_fail ? 1 : 0;
}
