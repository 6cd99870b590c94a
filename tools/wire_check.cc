// Stand-alone check of the host wire codec (csrc/tk_wire.cc) for sanitizer builds: the cases of
// tests/test_wire_codec.py restated in C++ with heap buffers of exactly the sizes the codec may
// touch, so that AddressSanitizer sees any byte read past a wire buffer or written outside a
// record, and UBSan any overflowing or misaligned access.  CPU only; never needs a device.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       -I include tools/wire_check.cc tachikoma_amd/csrc/tk_wire.cc -o wire_check && ./wire_check
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "tachikoma.h"

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

using Rec = std::vector<int32_t>;
static std::mt19937_64 g_rng(7);

static Rec span(int n, int64_t lo, uint64_t width) {
  Rec v(n);
  for (int i = 0; i < n; ++i) v[i] = (int32_t)(lo + (int64_t)(width == UINT64_MAX ? g_rng() : g_rng() % (width + 1)));
  for (int b = 0; b < n; b += 256) {
    v[b] = (int32_t)lo;
    if (b + 1 < n) v[b + 1] = (int32_t)(lo + (int64_t)width);
  }
  return v;
}

struct Case {
  std::vector<Rec> recs;
  std::vector<int> diff;
};

// Encodes into a heap buffer of tk_wire_bound bytes, copies the wire bytes into one of exactly
// their size, decodes into an image of exactly the layout's size; returns the decode status.
static int roundtrip(const Case& c, int threads, int corrupt = 0) {
  const int n = (int)c.recs.size();
  std::vector<tk_wire_record> r(n);
  int64_t at = 3;
  for (int i = 0; i < n; ++i) {
    r[i] = {at, (int64_t)c.recs[i].size(), c.diff[i], 0};
    at += 4 * (int64_t)c.recs[i].size() + 5;
  }
  const int64_t total = at;
  std::unique_ptr<uint8_t[]> src(new uint8_t[total]), out(new uint8_t[total]);
  std::memset(src.get(), 0xA5, total);
  for (int i = 0; i < n; ++i) std::memcpy(src.get() + r[i].offset, c.recs[i].data(), 4 * c.recs[i].size());
  std::memcpy(out.get(), src.get(), total);
  for (int i = 0; i < n; ++i) std::memset(out.get() + r[i].offset, 0, 4 * c.recs[i].size());
  const int64_t bound = tk_wire_bound(r.data(), n);
  CHECK(bound > 0);
  std::unique_ptr<uint8_t[]> big(new uint8_t[bound]);
  int64_t nb = tk_wire_encode_host(r.data(), n, src.get(), total, big.get(), bound);
  CHECK(nb > 0 && nb <= bound);
  if (corrupt == 1) nb -= 64;                        // truncated payload
  if (corrupt == 2) nb = 3;                          // truncated table
  std::unique_ptr<uint8_t[]> wire(new uint8_t[nb > 0 ? nb : 1]);
  std::memcpy(wire.get(), big.get(), nb);
  if (corrupt == 3) std::memset(wire.get(), 0xFF, 4);  // first segment starts far outside
  if (corrupt == 4) {  // a width code above 4 in the first segment (table of <= 16 segments: 64 B)
    const size_t nb0 = std::min<size_t>(64, (c.recs[0].size() + 255) / 256);
    wire[64 + ((4 * nb0 + 15) & ~(size_t)15)] = 9;
  }
  const int rc = tk_wire_decode(r.data(), n, wire.get(), nb, out.get(), total, threads);
  if (!corrupt) CHECK(rc == 0 && std::memcmp(out.get(), src.get(), total) == 0);
  return rc;
}

int main() {
  const int sizes[] = {1, 255, 256, 257, 3 * 256 + 17, 2 * 16384 + 300};
  for (int n : sizes) {
    std::vector<Case> cases;
    cases.push_back({{Rec(n, -77)}, {0}});
    for (uint64_t w : {255ull, 256ull, 65535ull, 65536ull, (1ull << 24) - 1, 1ull << 24})
      cases.push_back({{span(n, -100000, w)}, {0}});
    cases.push_back({{span(n, INT_MIN, 0xFFFFFFFFull)}, {0}});   // INT_MIN and INT_MAX in one block
    cases.push_back({{span(n, INT_MIN, UINT64_MAX)}, {0}});      // random full range
    cases.push_back({{Rec(n, INT_MIN), Rec(n, INT_MAX)}, {0, 1}});  // the difference wraps
    Rec a = span(n, -60000, 120000), b(n), c(n);
    for (int i = 0; i < n; ++i) b[i] = a[i] + i / 7 * 3 - 11, c[i] = b[i] + i / 7 * 3 - 11;
    cases.push_back({{a, b, c}, {0, 1, 1}});
    for (const Case& cs : cases)
      for (int threads : {1, 0}) roundtrip(cs, threads);
    for (int corrupt = 1; corrupt <= 4; ++corrupt) CHECK(roundtrip(cases.back(), 0, corrupt) == TK_ERR_INVALID_ARG);
  }
  {  // random full-range data: at most 1.03 x raw where the per-record constants are amortised
    const int n = 1 << 20;
    tk_wire_record r{1, n, 0, 0};
    CHECK(tk_wire_bound(&r, 1) <= (int64_t)(1.03 * 4 * n));
  }
  std::printf(g_fail ? "wire_check: %d failures\n" : "wire_check: ok (%d)\n", g_fail);
  return g_fail ? 1 : 0;
}
