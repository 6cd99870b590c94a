// Stand-alone check of the host wire codec (csrc/tk_wire.cc) for sanitizer builds: the cases of
// tests/test_wire_codec.py and tests/test_wire_codec8.py restated in C++ with heap buffers of exactly the sizes the codec may
// touch, so that AddressSanitizer sees any byte read past a wire buffer or written outside a
// record, and UBSan any overflowing or misaligned access; tk_wire_check, the host gate of the device
// decoder, is held to the decoder's verdict on every valid and damaged buffer; tk::wire_plan and
// tk::wire_seg_addr, which every encoder and decoder lays its records out with, are called
// directly.  CPU only; never needs a device.
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

#include "../tachikoma_amd/csrc/tk_wire.h"
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
  // the gate of the device decoder reads the table and the headers of the same exact-size buffer
  // and says what the decoder says
  CHECK(tk_wire_check(r.data(), n, wire.get(), nb) == rc);
  return rc;
}

// The same for records of any kind (kind 0: `data` holds int32 elements as bytes).  `corrupt`:
// 1 truncated payload, 5 the first segment's first block states width 2.  *wire_bytes: the size.
struct AnyRec {
  std::vector<uint8_t> data;
  int kind, diff;
};
static int roundtrip_any(const std::vector<AnyRec>& c, int threads, int corrupt = 0, int64_t* wire_bytes = nullptr) {
  const int n = (int)c.size();
  std::vector<tk_wire_record> r(n);
  int64_t at = 3;
  for (int i = 0; i < n; ++i) {
    const int64_t esize = c[i].kind ? 1 : 4;
    r[i] = {at, (int64_t)c[i].data.size() / esize, c[i].diff, c[i].kind};
    at += (int64_t)c[i].data.size() + 5;
  }
  const int64_t total = at;
  std::unique_ptr<uint8_t[]> src(new uint8_t[total]), out(new uint8_t[total]);
  std::memset(src.get(), 0xA5, total);
  for (int i = 0; i < n; ++i) std::memcpy(src.get() + r[i].offset, c[i].data.data(), c[i].data.size());
  std::memcpy(out.get(), src.get(), total);
  for (int i = 0; i < n; ++i) std::memset(out.get() + r[i].offset, 0x3C, c[i].data.size());
  const int64_t bound = tk_wire_bound(r.data(), n);
  CHECK(bound > 0);
  if (bound <= 0) return (int)bound;
  std::unique_ptr<uint8_t[]> big(new uint8_t[bound]);
  int64_t nb = tk_wire_encode_host(r.data(), n, src.get(), total, big.get(), bound);
  CHECK(nb > 0 && nb <= bound);
  if (wire_bytes) *wire_bytes = nb;
  if (corrupt == 1) nb -= 64;
  std::unique_ptr<uint8_t[]> wire(new uint8_t[nb > 0 ? nb : 1]);
  std::memcpy(wire.get(), big.get(), nb);
  if (corrupt == 5) {  // table of <= 16 segments: 64 B
    const size_t nb0 = std::min<size_t>(64, (c[0].data.size() / (c[0].kind ? 1 : 4) + 255) / 256);
    wire[64 + ((4 * nb0 + 15) & ~(size_t)15)] = 2;
  }
  const int rc = tk_wire_decode(r.data(), n, wire.get(), nb, out.get(), total, threads);
  if (!corrupt) CHECK(rc == 0 && std::memcmp(out.get(), src.get(), total) == 0);
  // the gate of the device decoder reads the table and the headers of the same exact-size buffer
  // and says what the decoder says
  CHECK(tk_wire_check(r.data(), n, wire.get(), nb) == rc);
  return rc;
}

static std::vector<uint8_t> random_bytes(int n, int lo, int hi) {  // values in [lo, hi] as int, stored as bytes
  std::vector<uint8_t> v(n);
  for (int i = 0; i < n; ++i) v[i] = (uint8_t)(lo + (int)(g_rng() % (uint64_t)(hi - lo + 1)));
  return v;
}
static std::vector<uint8_t> clamped(const std::vector<uint8_t>& p, int kind, int lo, int hi) {
  std::vector<uint8_t> v(p.size());
  for (size_t i = 0; i < p.size(); ++i) {
    const int x = kind == 1 ? (int)(int8_t)p[i] : (int)p[i];
    v[i] = (uint8_t)std::min(std::max(x, lo), hi);
  }
  return v;
}

// 1-byte records: plain (constant, random) and clamp-predicted pairs of both kinds, a pair with one
// element off by one in the last, short block (only that block goes raw), an int32 chain and a
// clamp pair in one buffer, and the refusals.
static void byte_cases(int n) {
  auto size_of = [&](int raw_blocks_bytes, int n_recs) {  // records of one segment each (n <= 16384)
    const int64_t nbk = (n + 255) / 256, hdr = ((4 * nbk + 15) & ~15) + ((nbk + 15) & ~15);
    return 64 + (n_recs - 1) * ((hdr + 63) & ~(int64_t)63) + ((hdr + raw_blocks_bytes + 63) & ~(int64_t)63);
  };
  for (int kind : {1, 2}) {
    const int lo_t = kind == 1 ? -128 : 0, hi_t = kind == 1 ? 127 : 255;
    const std::vector<uint8_t> prev = random_bytes(n, lo_t, hi_t);
    std::vector<std::vector<uint8_t>> recs;
    recs.push_back(clamped(prev, kind, lo_t + 128, hi_t));       // relu: only the lower bound is hit
    recs.push_back(clamped(prev, kind, lo_t + 60, hi_t - 70));   // both bounds (uint8: values above 127 on both sides)
    recs.push_back(prev);                                        // identity
    recs.push_back(clamped(prev, kind, lo_t, hi_t));             // bounds at the dtype's ends
    for (const auto& rec : recs)
      for (int threads : {1, 0}) {
        int64_t nb = 0;
        roundtrip_any({{prev, kind, 0}, {rec, kind, 1}}, threads, 0, &nb);
        if (n <= 16384 && n >= 256) CHECK(nb > (int64_t)n && nb < 2 * (int64_t)n);  // prev raw, rec predicted
      }
    {  // one element off by one, last in the final block: only that block is raw
      std::vector<uint8_t> rec = clamped(prev, kind, lo_t + 60, hi_t - 70);
      std::vector<uint8_t> c0(n, (uint8_t)7);
      rec[n - 1] = (uint8_t)(rec[n - 1] == (uint8_t)(lo_t + 60) ? rec[n - 1] + 1 : rec[n - 1] - 1);
      int64_t nb = 0;
      roundtrip_any({{c0, kind, 0}, {rec, kind, 1}}, 0, 0, &nb);
      // the constant predecessor cannot predict a block of two values, so compare against prev too
      roundtrip_any({{prev, kind, 0}, {rec, kind, 1}}, 0, 0, &nb);
      if (n <= 16384) {
        const int last = n - (n - 1) / 256 * 256;
        int64_t raw_prev = 0;
        for (int b = 0; b < n; b += 256) {
          const int cnt = std::min(256, n - b);
          if (!std::all_of(prev.begin() + b, prev.begin() + b + cnt, [&](uint8_t x) { return x == prev[b]; })) raw_prev += cnt;
        }
        const int64_t nbk = (n + 255) / 256, hdr = ((4 * nbk + 15) & ~15) + ((nbk + 15) & ~15);
        const bool last_const = last == 1;  // a one-element block is constant: width 0
        CHECK(nb == 64 + ((hdr + raw_prev + 63) & ~(int64_t)63) + ((hdr + (last_const ? 0 : last) + 63) & ~(int64_t)63));
      }
    }
    {  // plain records: constant (header only) and random (every block raw)
      int64_t nb = 0;
      roundtrip_any({{std::vector<uint8_t>(n, (uint8_t)0x91), kind, 0}}, 0, 0, &nb);
      if (n <= 16384) CHECK(nb == size_of(0, 1));
      roundtrip_any({{prev, kind, 0}}, 1);
    }
    {  // an int32 chain and a clamp pair in one buffer
      Rec a = span(n, -60000, 120000), b(n);
      for (int i = 0; i < n; ++i) b[i] = a[i] + i / 7 * 3 - 11;
      auto raw = [](const Rec& v) {
        std::vector<uint8_t> o(4 * v.size());
        std::memcpy(o.data(), v.data(), o.size());
        return o;
      };
      const std::vector<AnyRec> mix = {{raw(a), 0, 0}, {raw(b), 0, 1}, {prev, kind, 0}, {recs[1], kind, 1}};
      for (int threads : {1, 0}) roundtrip_any(mix, threads);
      CHECK(roundtrip_any(mix, 0, 1) == TK_ERR_INVALID_ARG);
    }
    CHECK(roundtrip_any({{prev, kind, 0}, {recs[1], kind, 1}}, 0, 5) == TK_ERR_INVALID_ARG);
    CHECK(roundtrip_any({{prev, kind, 0}, {recs[1], kind, 1}}, 0, 1) == TK_ERR_INVALID_ARG);
    // a clamp record whose predecessor has another size or kind
    tk_wire_record bad[2] = {{3, n, 0, kind}, {3 + n + 5, n, 1, 3 - kind}};
    CHECK(tk_wire_bound(bad, 2) == TK_ERR_INVALID_ARG);
    bad[1].kind = kind, bad[0].n_elems = n + 1;
    CHECK(tk_wire_bound(bad, 2) == TK_ERR_INVALID_ARG);
    bad[0].n_elems = n, bad[0].kind = 0;
    CHECK(tk_wire_bound(bad, 2) == TK_ERR_INVALID_ARG);
    bad[0].kind = 7, bad[1].diff = 0;
    CHECK(tk_wire_bound(bad, 2) == TK_ERR_INVALID_ARG);
  }
}

// Bias coding: a chain a, a + bias1[c], a + bias1[c] + bias2[c], ... of `planes * channels * samples`
// elements, every record after the first coded with its addend, the addends in heap buffers of
// exactly `channels` elements.  `junk`: the last record is noise instead (the prediction fails).
// Returns the wire bytes; *flat: those of the same chain if every coded block were constant.
static int64_t bias_roundtrip(int plane, int channels, int samples, const std::vector<Rec>& biases, bool junk, int threads,
                              int64_t* flat) {
  const int64_t n = (int64_t)plane * channels * samples;
  const int k = 1 + (int)biases.size();
  std::vector<Rec> recs(k, Rec(n));
  recs[0] = span((int)n, -60000, 120000);
  std::vector<std::unique_ptr<int32_t[]>> addends;
  for (int m = 1; m < k; ++m) {
    addends.emplace_back(new int32_t[channels]);
    std::memcpy(addends.back().get(), biases[m - 1].data(), 4 * (size_t)channels);
    for (int64_t e = 0; e < n; ++e)
      recs[m][e] = junk && m == k - 1 ? (int32_t)g_rng()
                                      : (int32_t)((uint32_t)recs[m - 1][e] + (uint32_t)biases[m - 1][(e / plane) % channels]);
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
  std::memcpy(out.get(), src.get(), total);
  for (int m = 0; m < k; ++m) std::memset(out.get() + r[m].offset, 0, 4 * n);
  const int64_t bound = tk_wire_bound(r.data(), k);
  CHECK(bound > 0);
  if (bound <= 0) return bound;
  std::unique_ptr<uint8_t[]> big(new uint8_t[bound]);
  const int64_t nb = tk_wire_encode_host_bias(r.data(), ad.data(), k, src.get(), total, big.get(), bound);
  CHECK(nb > 0 && nb <= bound);
  if (nb <= 0) return nb;
  std::unique_ptr<uint8_t[]> wire(new uint8_t[nb]);
  std::memcpy(wire.get(), big.get(), nb);
  CHECK(tk_wire_decode_bias(r.data(), ad.data(), k, wire.get(), nb, out.get(), total, threads) == 0 &&
        std::memcmp(out.get(), src.get(), total) == 0);
  // packed trace files do not code addends, and the entry points without addends cannot: all
  // refuse the bias-coded records
  CHECK(tk_wire_check(r.data(), k, wire.get(), nb) == TK_ERR_UNSUPPORTED);
  CHECK(tk_wire_decode(r.data(), k, wire.get(), nb, out.get(), total, threads) == TK_ERR_UNSUPPORTED);
  CHECK(tk_wire_encode_host(r.data(), k, src.get(), total, big.get(), bound) == TK_ERR_UNSUPPORTED);
  // the first record alone, then headers only for each record after it
  int64_t first = 0, hdrs = 0, n_seg = 0;
  {
    tk_wire_record r0 = r[0];
    first = tk_wire_encode_host(&r0, 1, src.get(), total, big.get(), bound);
    for (int64_t e = 0; e < n; e += tk::kWireSegElems, ++n_seg)
      hdrs += tk::wire_align(tk::wire_header_bytes((int)((std::min<int64_t>(tk::kWireSegElems, n - e) + 255) / 256)), 64);
    first -= tk::wire_table_bytes(n_seg);
  }
  *flat = tk::wire_table_bytes(k * n_seg) + first + (k - 1) * hdrs;
  return nb;
}

static void bias_cases() {
  auto bias = [](int channels, int64_t scale) {
    Rec b(channels);
    for (int c = 0; c < channels; ++c) b[c] = (int32_t)((c * 7919 % channels) * scale - 30000);
    return b;
  };
  int64_t flat = 0;
  for (int threads : {1, 0}) {
    // 7x7 planes, where every block straddles: the pair costs its headers alone
    CHECK(bias_roundtrip(49, 24, 2, {bias(24, 1013)}, false, threads, &flat) == flat);
    // a plane longer than a segment: segments 1 and 2 start mid-plane; a ragged last block
    CHECK(bias_roundtrip(16385, 2, 1, {bias(2, 999)}, false, threads, &flat) == flat);
    // dense (plane 1), and planes below a lane's 16 elements
    CHECK(bias_roundtrip(1, 10, 5, {bias(10, 31)}, false, threads, &flat) == flat);
    CHECK(bias_roundtrip(3, 5, 40, {bias(5, 31)}, false, threads, &flat) == flat);
    // a chain of three with addends at both ends of int32: sums and differences wrap
    CHECK(bias_roundtrip(196, 4, 3, {{INT_MIN, INT_MAX, -1, 0}, {INT_MAX, INT_MAX, INT_MIN, 5}}, false, threads, &flat) == flat);
    // the prediction fails everywhere: still round-trips, at the raw width
    CHECK(bias_roundtrip(49, 24, 20, {bias(24, 1013), bias(24, 77)}, true, threads, &flat) >= flat + 4 * 49 * 24 * 20);
  }
  // a bias-coded record that is not differenced, follows a 1-byte record, or lacks its geometry
  const int32_t one[1] = {1};
  tk_wire_record bad[2] = {{0, 8, 0, 0}, {32, 8, 1, 3}};
  tk_wire_addend ad[2] = {{0, 0, nullptr}, {1, 1, one}};
  uint8_t image[64] = {0}, wire[1024];
  auto encode = [&] { return tk_wire_encode_host_bias(bad, ad, 2, image, 64, wire, sizeof(wire)); };
  CHECK(tk_wire_bound(bad, 2) > 0 && tk_wire_bound(bad, 2) <= (int64_t)sizeof(wire) && encode() > 0);
  bad[1].diff = 0;
  CHECK(tk_wire_bound(bad, 2) == TK_ERR_INVALID_ARG && encode() == TK_ERR_INVALID_ARG);
  bad[1].diff = 1, ad[1].plane = 0;
  CHECK(encode() == TK_ERR_INVALID_ARG);
  ad[1].plane = 1, ad[1].channels = 0;
  CHECK(encode() == TK_ERR_INVALID_ARG);
  ad[1].channels = 1, ad[1].addend = nullptr;
  CHECK(encode() == TK_ERR_INVALID_ARG);
  ad[1].addend = one, bad[0].kind = 1;
  CHECK(tk_wire_bound(bad, 2) == TK_ERR_INVALID_ARG && encode() == TK_ERR_INVALID_ARG);
}

// tk::wire_plan refuses `r` with `status`, under the caller's name
static bool refused(const std::vector<tk_wire_record>& r, int64_t image_bytes, int status = TK_ERR_INVALID_ARG) {
  tk::WirePlan p;
  tk::g_err.clear();
  return tk::wire_plan(r.data(), (int)r.size(), image_bytes, "some_caller", &p) == status &&
         tk::g_err.rfind("some_caller: ", 0) == 0;
}

// The planner every encoder and decoder lays its records out with, and the address helper.
static void planner_cases() {
  const int seg = tk::kWireSegElems;
  {  // a chain of three int32 records, one element longer than a segment
    const int64_t n = seg + 1;
    const std::vector<tk_wire_record> r = {{0, n, 0, 0}, {4 * n, n, 1, 0}, {8 * n, n, 1, 0}};
    tk::WirePlan p;
    CHECK(tk::wire_plan(r.data(), 3, 12 * n, "t", &p) == TK_OK);
    CHECK(p.segs.size() == 6 && p.units.size() == 2);
    for (size_t i = 0; i < p.segs.size(); ++i)
      CHECK(p.segs[i].rec == (int)i / 2 && p.segs[i].n == (i % 2 ? 1 : seg) && p.segs[i].e0 == (int64_t)(i % 2) * seg);
    for (size_t u = 0; u < p.units.size(); ++u)
      CHECK(p.units[u].first == (int)u && p.units[u].stride == 2 && p.units[u].count == 3);
    CHECK(p.bound == tk_wire_bound(r.data(), 3));
    CHECK(p.bound == 64 + 3 * (tk::wire_seg_bound(seg) + tk::wire_seg_bound(1)));
    CHECK(refused(r, 12 * n - 1));  // the last record's extent leaves the image
    // the helper: byte offsets of 4-byte elements; a null base gives null
    std::vector<char> rec(4 * n), prev(4 * n);
    if (p.segs.size() == 6) {
      const tk::WireSegAddr a = tk::wire_seg_addr(p.segs[3], 0, rec.data(), prev.data());
      CHECK(a.at == rec.data() + 4 * (int64_t)seg && a.prev == prev.data() + 4 * (int64_t)seg);
      const tk::WireSegAddr b = tk::wire_seg_addr(p.segs[3], 0, nullptr, nullptr);
      CHECK(b.at == nullptr && b.prev == nullptr);
    }
  }
  {  // chains cut by a record of another kind: int32, int8 and uint8 in one plan
    const int64_t n = seg + 5, m = 300;
    const std::vector<tk_wire_record> r = {{0, n, 0, 0}, {0, n, 1, 0}, {0, m, 0, 1}, {0, m, 1, 1}, {0, m, 0, 2}, {0, n, 0, 0}};
    tk::WirePlan p;
    CHECK(tk::wire_plan(r.data(), 6, -1, "t", &p) == TK_OK);
    const int want_rec[9] = {0, 0, 1, 1, 2, 3, 4, 5, 5};
    const int want_n[9] = {seg, 5, seg, 5, 300, 300, 300, seg, 5};
    CHECK(p.segs.size() == 9);
    for (size_t i = 0; i < p.segs.size() && i < 9; ++i)
      CHECK(p.segs[i].rec == want_rec[i] && p.segs[i].n == want_n[i] && p.segs[i].e0 == (want_n[i] == 5 ? seg : 0));
    const tk::WireUnit want_units[6] = {{0, 2, 2}, {1, 2, 2}, {4, 1, 2}, {6, 1, 1}, {7, 2, 1}, {8, 2, 1}};
    CHECK(p.units.size() == 6);
    for (size_t u = 0; u < p.units.size() && u < 6; ++u)
      CHECK(p.units[u].first == want_units[u].first && p.units[u].stride == want_units[u].stride &&
            p.units[u].count == want_units[u].count);
    CHECK(p.bound == tk_wire_bound(r.data(), 6));
    CHECK(p.bound == 64 + 3 * (tk::wire_seg_bound(seg) + tk::wire_seg_bound(5)) + 3 * tk::wire_seg_bound(300, 1));
  }
  {  // an unchained 1-byte record whose predecessor another plan holds: the helper still gives the
     // predecessor's address, the units do not chain it
    const int64_t n = seg + 10;
    const tk_wire_record r{0, n, 0, 2};
    tk::WirePlan p;
    CHECK(tk::wire_plan(&r, 1, -1, "t", &p) == TK_OK);
    CHECK(p.segs.size() == 2 && p.units.size() == 2);
    for (size_t u = 0; u < p.units.size(); ++u) CHECK(p.units[u].first == (int)u && p.units[u].count == 1);
    std::vector<char> rec(n), prev(n);
    if (p.segs.size() == 2) {
      const tk::WireSegAddr a = tk::wire_seg_addr(p.segs[1], r.kind, rec.data(), prev.data());
      CHECK(a.at == rec.data() + seg && a.prev == prev.data() + seg);
      CHECK(tk::wire_seg_addr(p.segs[1], r.kind, rec.data(), nullptr).prev == nullptr);
    }
  }
  // the refusals, each under the caller's name
  CHECK(refused({{0, 8, 1, 0}}, -1));                                  // record 0 with diff
  CHECK(refused({{0, 8, 0, 0}, {32, 9, 1, 0}}, -1));                   // diff across a change of size
  CHECK(refused({{0, 8, 0, 1}, {8, 8, 1, 2}}, -1));                    // ... of kind
  CHECK(refused({{0, 0, 0, 0}}, -1));                                  // no elements
  CHECK(refused({{0, ((int64_t)1 << 40) + 1, 0, 1}}, -1));             // too many
  CHECK(refused({{0, 8, 0, 4}}, -1) && refused({{0, 8, 0, -1}}, -1));  // unknown kinds
  CHECK(refused({{0, 8, 0, 0}, {32, 8, 1, 3}}, -1, TK_ERR_UNSUPPORTED));   // bias-coded, and no addends taken
  CHECK(refused({{-1, 8, 0, 0}}, -1) && refused({{-1, 8, 0, 0}}, 64));
  CHECK(refused({{65, 8, 0, 1}}, 64));                                 // an offset outside the image
  CHECK(refused({{36, 8, 0, 0}}, 64) && !refused({{32, 8, 0, 0}}, 64));  // an extent outside it
  CHECK(refused({}, -1));
  // 2^31 segments: refused before anything is laid out
  CHECK(refused(std::vector<tk_wire_record>(32, tk_wire_record{0, (int64_t)1 << 40, 0, 1}), -1, TK_ERR_UNSUPPORTED));
}

int main() {
  planner_cases();
  bias_cases();
  for (int n : {1, 15, 16, 17, 255, 256, 257, 3 * 256 + 17, 2 * 16384 + 300}) byte_cases(n);
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
