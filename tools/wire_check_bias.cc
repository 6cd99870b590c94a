// Stand-alone check of tk_wire_check_bias (csrc/tk_wire.cc), the host gate of the device decoder
// for packed trace files of version 3, for sanitizer builds.  It follows tools/wire_check.cc: bias
// chains over the grid of tests/wire_cases_bias.py are encoded by tk_wire_encode_host_bias, the wire
// bytes copied into a heap buffer of exactly their size, and on that buffer -- whole, cut short,
// and damaged in its table and headers -- the gate must say exactly what tk_wire_decode_bias says.
// While the gate runs, every block payload of the buffer is poisoned and every addend pointer
// dangles (freed heap memory): AddressSanitizer reports a payload byte or an addend value it reads,
// as it reports any byte read outside the buffer.  CPU only; never needs a device.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       -I include tools/wire_check_bias.cc tachikoma_amd/csrc/tk_wire.cc -o wire_check_bias && ./wire_check_bias
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../tachikoma_amd/csrc/tk_wire.h"
#include "tachikoma.h"

#if defined(__SANITIZE_ADDRESS__)
#define TK_ASAN 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define TK_ASAN 1
#endif
#endif
#ifdef TK_ASAN
#include <sanitizer/asan_interface.h>
#define POISON(p, n) __asan_poison_memory_region((p), (n))
#define UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#else
#define POISON(p, n) ((void)(p), (void)(n))
#define UNPOISON(p, n) ((void)(p), (void)(n))
#endif

namespace tk {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace tk

static int g_fail = 0, g_checks = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    ++g_checks;                                                   \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);     \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

using Rec = std::vector<int32_t>;
static std::mt19937_64 g_rng(11);

// The block payloads of a wire buffer the decoder accepted: (offset, length) of each segment's bytes
// behind its header.
static std::vector<std::pair<int64_t, int64_t>> payloads(const tk_wire_record* r, int k, const uint8_t* wire,
                                                         int64_t wire_bytes) {
  tk::WirePlan p;
  std::vector<std::pair<int64_t, int64_t>> out;
  tk_wire_addend none{1, 1, reinterpret_cast<const int32_t*>(wire)};  // admission only: nothing is read through it
  std::vector<tk_wire_addend> ad((size_t)k, none);
  if (tk::wire_plan(r, k, -1, "payloads", &p, ad.data()) != TK_OK) return out;
  const int64_t table = tk::wire_table_bytes((int64_t)p.segs.size());
  for (size_t i = 0; i < p.segs.size(); ++i) {
    uint32_t start;
    std::memcpy(&start, wire + 4 * i, 4);
    const int64_t len = tk::wire_seg_extent(tk::wire_seg_kind(r[p.segs[i].rec].kind), p.segs[i].n, start,
                                            (const char*)wire + table, wire_bytes - table);
    const int64_t hdr = tk::wire_header_bytes((p.segs[i].n + tk::kWireBlock - 1) / tk::kWireBlock);
    if (len > hdr) out.push_back({table + 64 * (int64_t)start + hdr, len - hdr});
  }
  return out;
}

// A chain a, a + bias1[c], ... coded with its addends; the gate against the decoder on the whole
// buffer and on each damaged copy.  `junk`: the last record is noise, so its blocks have payloads.
static void chain(int plane, int channels, int samples, int links, bool junk) {
  const int64_t n = (int64_t)plane * channels * samples;
  const int k = 1 + links;
  std::vector<Rec> recs(k, Rec(n));
  for (auto& x : recs[0]) x = (int32_t)(g_rng() % 120001) - 60000;
  std::vector<std::unique_ptr<int32_t[]>> addends;
  for (int m = 1; m < k; ++m) {
    addends.emplace_back(new int32_t[channels]);  // exactly `channels` values
    for (int c = 0; c < channels; ++c)
      addends.back()[c] = c == 0 ? INT_MIN : c == 1 ? INT_MAX : (int32_t)(g_rng() % 60001) - 30000;
    for (int64_t e = 0; e < n; ++e)
      recs[m][e] = junk && m == k - 1 ? (int32_t)g_rng()
                                      : (int32_t)((uint32_t)recs[m - 1][e] + (uint32_t)addends.back()[(e / plane) % channels]);
  }
  std::vector<tk_wire_record> r(k);
  std::vector<tk_wire_addend> ad(k);
  int64_t at = 3;
  for (int m = 0; m < k; ++m) {
    r[m] = {at, n, m > 0, m ? 3 : 0};
    ad[m] = {m ? plane : 0, m ? channels : 0, m ? addends[m - 1].get() : nullptr};
    at += 4 * n + 5;
  }
  const int64_t total = at;
  std::unique_ptr<uint8_t[]> src(new uint8_t[total]), out(new uint8_t[total]);
  std::memset(src.get(), 0xA5, total);
  for (int m = 0; m < k; ++m) std::memcpy(src.get() + r[m].offset, recs[m].data(), 4 * n);
  const int64_t bound = tk_wire_bound(r.data(), k);
  CHECK(bound > 0);
  if (bound <= 0) return;
  std::unique_ptr<uint8_t[]> big(new uint8_t[bound]);
  const int64_t used = tk_wire_encode_host_bias(r.data(), ad.data(), k, src.get(), total, big.get(), bound);
  CHECK(used > 0 && used <= bound);
  if (used <= 0) return;
  // the addends the gate is given: the same geometry, pointers into memory that has been freed
  std::vector<tk_wire_addend> dangling = ad;
  for (int m = 1; m < k; ++m) {
    int32_t* gone = new int32_t[channels];
    dangling[m].addend = gone;
    delete[] gone;
  }
  tk::WirePlan plan;
  CHECK(tk::wire_plan(r.data(), k, -1, "chain", &plan, ad.data()) == TK_OK);
  const int64_t n_seg = (int64_t)plan.segs.size(), table = tk::wire_table_bytes(n_seg);
  const int seg = (int)(n_seg - 1);  // a segment of the last (bias-coded) record
  uint32_t seg_start;
  std::memcpy(&seg_start, big.get() + 4 * seg, 4);
  const int nb = (plan.segs[seg].n + tk::kWireBlock - 1) / tk::kWireBlock;
  const int64_t widths_at = table + 64 * (int64_t)seg_start + tk::wire_align(4 * (int64_t)nb, 16);
  // damage: 0 none, 1 one byte short of the last segment's stated end, 2 64 bytes short, 3 a cut
  // table, 4 a start beyond the payload, 5 a width of 5, 6 a width of 255, 7 an empty buffer
  for (int damage = 0; damage <= 7; ++damage) {
    int64_t nbytes = used;
    if (damage == 1) {
      const int64_t len = tk::wire_seg_extent(tk::kWireI32, plan.segs[seg].n, seg_start, (const char*)big.get() + table,
                                              used - table);
      CHECK(len > 0);
      nbytes = table + 64 * (int64_t)seg_start + len - 1;
    }
    if (damage == 2) nbytes = used - 64;
    if (damage == 3) nbytes = table - 1;
    if (damage == 7) nbytes = 0;
    std::unique_ptr<uint8_t[]> wire(new uint8_t[nbytes > 0 ? nbytes : 1]);  // exactly the stated size
    std::memcpy(wire.get(), big.get(), nbytes);
    if (damage == 4) {
      const uint32_t far = (uint32_t)((used - table) / 64 + 1);
      std::memcpy(wire.get() + 4 * seg, &far, 4);
    }
    if (damage == 5) wire[widths_at] = 5;
    if (damage == 6) wire[widths_at + nb - 1] = 255;
    std::memcpy(out.get(), src.get(), total);
    const int want = tk_wire_decode_bias(r.data(), ad.data(), k, wire.get(), nbytes, out.get(), total, damage % 2);
    if (damage == 0) CHECK(want == TK_OK && std::memcmp(out.get(), src.get(), total) == 0);
    else CHECK(want == TK_ERR_INVALID_ARG);
    // the gate: no payload byte (poisoned where the buffer parses) and no addend value (freed)
    const auto pay = want == TK_OK ? payloads(r.data(), k, wire.get(), nbytes) : std::vector<std::pair<int64_t, int64_t>>();
    if (junk && damage == 0) CHECK(!pay.empty());
    for (const auto& pr : pay) POISON(wire.get() + pr.first, (size_t)pr.second);
    const int got = tk_wire_check_bias(r.data(), dangling.data(), k, wire.get(), nbytes);
    for (const auto& pr : pay) UNPOISON(wire.get() + pr.first, (size_t)pr.second);
    CHECK(got == want);
  }
  // the records' rules are the decoder's too: without addends, and with a broken addend entry
  std::unique_ptr<uint8_t[]> wire(new uint8_t[used]);
  std::memcpy(wire.get(), big.get(), used);
  CHECK(tk_wire_check_bias(r.data(), nullptr, k, wire.get(), used) == TK_ERR_UNSUPPORTED);
  CHECK(tk_wire_decode_bias(r.data(), nullptr, k, wire.get(), used, out.get(), total, 1) == TK_ERR_UNSUPPORTED);
  CHECK(tk_wire_check(r.data(), k, wire.get(), used) == TK_ERR_UNSUPPORTED);
  for (int what = 0; what < 4; ++what) {
    std::vector<tk_wire_addend> bad = ad;
    std::vector<tk_wire_record> rb = r;
    if (what == 0) bad[1].plane = 0;
    if (what == 1) bad[1].channels = 0;
    if (what == 2) bad[1].addend = nullptr;
    if (what == 3) rb[1].diff = 0;
    const int want = tk_wire_decode_bias(rb.data(), bad.data(), k, wire.get(), used, out.get(), total, 1);
    CHECK(want == TK_ERR_INVALID_ARG && tk_wire_check_bias(rb.data(), bad.data(), k, wire.get(), used) == want);
  }
}

int main() {
  // (plane, channels, samples) of tests/wire_cases_bias.py, the ragged end, and more than one segment
  // with a plane below a block
  const int grid[][3] = {{1, 10, 5}, {3, 5, 40}, {7, 24, 3}, {49, 24, 2}, {81, 8, 3}, {196, 4, 3}, {256, 3, 2},
                         {257, 3, 2}, {16385, 2, 1}, {1, 157, 5}, {49, 24, 30}};
  for (const auto& g : grid)
    for (int junk = 0; junk <= 1; ++junk) chain(g[0], g[1], g[2], 1, junk != 0);
  chain(196, 4, 3, 2, false);  // the chain of three
  chain(196, 4, 3, 2, true);
#ifndef TK_ASAN
  std::printf("wire_check_bias: built without AddressSanitizer, the reads are not watched\n");
#endif
  std::printf(g_fail ? "wire_check_bias: %d failures\n" : "wire_check_bias: ok (%d checks)\n", g_fail ? g_fail : g_checks);
  return g_fail ? 1 : 0;
}
