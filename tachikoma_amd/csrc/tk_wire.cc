// Host side of the trace wire format (tk_wire.h): the planner every encoder and decoder lays its
// records out with, the decoder that widens a wire buffer into the trace image (and rebuilds
// clamp-predicted 1-byte records from the image bytes before them, and bias-coded int32 records
// one channel run at a time) on a fixed thread pool, and a
// reference encoder so the decoder is testable without a device.  Plain C++ (no HIP): also
// compiled alone into the sanitizer check of tools/wire_check.cc.
#include "tk_wire.h"

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>

#include "tk_tensor.h"

namespace tk {

int wire_plan(const tk_wire_record* recs, int n_recs, int64_t image_bytes, const char* who, WirePlan* p,
              const tk_wire_addend* addends, bool bias_ok) {
  if (!recs || n_recs < 1) {
    set_error(std::string(who) + ": no records");
    return TK_ERR_INVALID_ARG;
  }
  int64_t n_seg = 0;
  for (int i = 0; i < n_recs; ++i) {
    const int kind = recs[i].kind;
    if (kind == kWireI32Bias &&
        (!recs[i].diff || recs[i].n_elems >= ((int64_t)1 << 31) ||
         (addends && (!addends[i].addend || addends[i].plane < 1 || addends[i].channels < 1)))) {
      set_error(std::string(who) + ": record " + std::to_string(i) +
                " is bias-coded (kind 3) but is not a differenced record of fewer than 2^31 elements with an addend "
                "and a plane and channels of at least 1");
      return TK_ERR_INVALID_ARG;
    }
    if (kind == kWireI32Bias && !addends && !bias_ok) {
      set_error(std::string(who) + ": record " + std::to_string(i) +
                " is bias-coded (kind 3), which this entry point takes no addends for (packed trace files, format "
                "version 2, and the device decoder do not code them)");
      return TK_ERR_UNSUPPORTED;
    }
    const int64_t esize = wire_elem_bytes(kind);
    const bool inside = kind >= kWireI32 && kind <= kWireI32Bias && recs[i].offset >= 0 && recs[i].n_elems >= 1 &&
                        recs[i].n_elems <= ((int64_t)1 << 40) &&
                        (image_bytes < 0 ||
                         (recs[i].offset <= image_bytes && esize * recs[i].n_elems <= image_bytes - recs[i].offset));
    if (!inside || (recs[i].diff && (i == 0 || recs[i - 1].n_elems != recs[i].n_elems ||
                                     wire_seg_kind(recs[i - 1].kind) != wire_seg_kind(kind)))) {
      set_error(std::string(who) + ": record " + std::to_string(i) +
                " is of no known kind, lies outside the image or follows (diff) a record of another size or kind");
      return TK_ERR_INVALID_ARG;
    }
    n_seg += (recs[i].n_elems + kWireSegElems - 1) / kWireSegElems;
  }
  if (n_seg >= ((int64_t)1 << 31)) {  // segment indices are 32-bit, on the host and on the device
    set_error(std::string(who) + ": too many segments");
    return TK_ERR_UNSUPPORTED;
  }
  p->segs.clear(), p->units.clear();
  p->segs.reserve((size_t)n_seg);
  p->bound = wire_table_bytes(n_seg);
  int r = 0;
  while (r < n_recs) {
    int k = 1;  // records r .. r + k - 1 form a chain
    while (r + k < n_recs && recs[r + k].diff) ++k;
    const int64_t n = recs[r].n_elems;
    const int64_t S = (n + kWireSegElems - 1) / kWireSegElems;
    const int64_t first = (int64_t)p->segs.size();
    for (int m = 0; m < k; ++m)
      for (int64_t j = 0; j < S; ++j) {
        const int32_t sn = (int32_t)std::min<int64_t>(kWireSegElems, n - j * kWireSegElems);
        p->segs.push_back({r + m, sn, j * kWireSegElems});
        p->bound += wire_seg_bound(sn, wire_elem_bytes(recs[r].kind));
      }
    for (int64_t j = 0; j < S; ++j) p->units.push_back({(int32_t)(first + j), (int32_t)S, k});
    r += k;
  }
  return TK_OK;
}

// ---------------------------------------------------------------- thread pool
// Sized once from the process's CPU affinity mask (never the machine's core count), at most 16;
// TK_WIRE_THREADS overrides (1..16).  DESIGN.md section 8 has the measured rates per thread count
// and placement.  Work items are claimed from an atomic counter; the caller waits and does not
// decode itself (it is a HIP host-function thread).  The pool is never torn down: its threads
// sleep between jobs and end with the process.
namespace {
class Pool {
 public:
  static Pool& get() {
    static Pool* p = new Pool();
    return *p;
  }
  int size() const { return n_; }
  // fn(i) for i in [0, count) on up to `threads` workers; returns when all are done
  template <typename F>
  void run(int64_t count, int threads, F&& fn) {
    std::lock_guard<std::mutex> job(job_mu_);  // one job at a time
    struct Ctx {
      F* fn;
    } ctx{&fn};
    {
      std::lock_guard<std::mutex> lk(mu_);
      call_ = [](void* c, int64_t i) { (*static_cast<Ctx*>(c)->fn)(i); };
      ctx_ = &ctx;
      count_ = count;
      next_.store(0, std::memory_order_relaxed);
      limit_ = threads > 0 ? std::min(threads, n_) : n_;
      active_ = limit_;
      ++gen_;
    }
    cv_.notify_all();
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [&] { return active_ == 0; });
  }

 private:
  Pool() {
    int n = 0;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
    n = std::max(1, std::min(n, 16));
    if (const char* e = std::getenv("TK_WIRE_THREADS")) {
      const int v = std::atoi(e);
      if (v >= 1 && v <= 16) n = v;
    }
    n_ = n;
    for (int t = 0; t < n_; ++t) std::thread([this, t] { worker(t); }).detach();
  }
  void worker(int id) {
    uint64_t seen = 0;
    for (;;) {
      void (*call)(void*, int64_t);
      void* ctx;
      int64_t count;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return gen_ != seen; });
        seen = gen_;
        if (id >= limit_) continue;
        call = call_, ctx = ctx_, count = count_;
      }
      for (int64_t i; (i = next_.fetch_add(1, std::memory_order_relaxed)) < count;) call(ctx, i);
      std::lock_guard<std::mutex> lk(mu_);
      if (--active_ == 0) done_cv_.notify_all();
    }
  }
  int n_ = 1;
  std::mutex job_mu_, mu_;
  std::condition_variable cv_, done_cv_;
  uint64_t gen_ = 0;
  void (*call_)(void*, int64_t) = nullptr;
  void* ctx_ = nullptr;
  int64_t count_ = 0;
  int limit_ = 0, active_ = 0;
  std::atomic<int64_t> next_{0};
};

// ---------------------------------------------------------------- decoder
// image words are read and written through memcpy: NDArray-list payload offsets are 8-byte
// aligned only by layout, and the decoder promises nothing about alignment at all
// A: a bias-coded block that holds more than one channel run takes its constant per element from
// `add` (base + the element's addend, laid out by the caller) instead of from `base`
template <int W, bool D, bool A>
void widen(char* dst, const char* prev, const uint8_t* p, int cnt, uint32_t base, const uint32_t* add) {
  for (int i = 0; i < cnt; ++i) {
    uint32_t v = A ? add[i] : base;
    if (W >= 1) v += p[i];
    if (W >= 2) v += (uint32_t)p[cnt + i] << 8;
    if (W >= 3) v += (uint32_t)p[2 * cnt + i] << 16;
    if (W >= 4) v += (uint32_t)p[3 * cnt + i] << 24;
    if (D) {
      uint32_t q;
      std::memcpy(&q, prev + 4 * (int64_t)i, 4);
      v += q;
    }
    std::memcpy(dst + 4 * (int64_t)i, &v, 4);
  }
}
template <bool D, bool A = false>
void widen_w(int w, char* dst, const char* prev, const uint8_t* p, int cnt, uint32_t base, const uint32_t* add = nullptr) {
  switch (w) {
    case 0: return widen<0, D, A>(dst, prev, p, cnt, base, add);
    case 1: return widen<1, D, A>(dst, prev, p, cnt, base, add);
    case 2: return widen<2, D, A>(dst, prev, p, cnt, base, add);
    case 3: return widen<3, D, A>(dst, prev, p, cnt, base, add);
    default: return widen<4, D, A>(dst, prev, p, cnt, base, add);
  }
}

// The channel runs of a bias-coded segment (tk_wire.h): a cursor over its elements that knows the
// channel of the element it stands on and how many elements are left in that channel's plane.
struct BiasWalk {
  const int32_t* addend;
  int32_t plane, channels, c, r;
  explicit BiasWalk(const WireBias& b) : addend(b.addend), plane(b.plane), channels(b.channels), c(b.c0), r(b.r0) {}
  int run(int left) const { return std::min(left, plane - r); }  // elements up to the plane's end
  uint32_t value() const { return (uint32_t)addend[c]; }
  void advance(int k) {  // k <= run()
    if ((r += k) == plane) r = 0, c = c + 1 == channels ? 0 : c + 1;
  }
};

// 1-byte blocks: dst = clamp(prev, lo, hi) in the record's dtype, 32 bytes at a time.  int8 is
// compared as uint8 with the sign bit flipped (`flip` 0x80; lo and hi come flipped already), so
// both dtypes are one unsigned byte min / max, which the compiler keeps in vector registers.
inline uint8_t clamp_u8(uint8_t x, uint8_t lo, uint8_t hi) {
  x = x < lo ? lo : x;
  return x > hi ? hi : x;
}
void clamp_block(char* dst, const char* prev, int cnt, uint8_t lo, uint8_t hi, uint8_t flip) {
  int i = 0;
  for (; i + 32 <= cnt; i += 32) {
    uint8_t v[32];
    std::memcpy(v, prev + i, 32);
    for (int j = 0; j < 32; ++j) v[j] = (uint8_t)(clamp_u8((uint8_t)(v[j] ^ flip), lo, hi) ^ flip);
    std::memcpy(dst + i, v, 32);
  }
  for (; i < cnt; ++i) dst[i] = (char)(clamp_u8((uint8_t)((uint8_t)prev[i] ^ flip), lo, hi) ^ flip);
}

}  // namespace

// The extent of a segment of n elements of `kind` whose table entry is `start`: its unrounded
// length by the widths its header states, or -1 if its start, its header or that length does not
// lie inside the payload, or a width is not one the kind allows.  Reads the header only.  The host
// decoder, tk_wire_check and (restated for the device) the decode kernel hold a segment to this.
int64_t wire_seg_extent(int kind, int n, uint32_t start, const char* payload, int64_t payload_bytes) {
  const int64_t off = (int64_t)start * 64;
  const int nb = (n + kWireBlock - 1) / kWireBlock;
  const int64_t hdr = wire_header_bytes(nb);
  if (off > payload_bytes || hdr > payload_bytes - off) return -1;
  const uint8_t* widths = (const uint8_t*)payload + off + wire_align(4 * (int64_t)nb, 16);
  int64_t len = hdr;
  const int max_w = kind == kWireI32 ? 4 : 1;
  for (int b = 0; b < nb; ++b) {
    if (widths[b] > max_w) return -1;
    len += (int64_t)widths[b] * std::min(kWireBlock, n - b * kWireBlock);
  }
  return len > payload_bytes - off ? -1 : len;
}

namespace {
// Decodes segment i; returns its length rounded to 64 B, or -1 if it does not lie inside the
// payload (nothing past the payload is read, nothing outside the segment's record is written).
int64_t decode_seg(const WireJob& j, int64_t i, const char* payload, int64_t payload_bytes) {
  const WireSegHost& sg = j.segs[i];
  uint32_t start;
  std::memcpy(&start, j.wire + 4 * i, 4);
  const int64_t len = wire_seg_extent(sg.kind, sg.n, start, payload, payload_bytes);
  if (len < 0) return -1;
  const int nb = (sg.n + kWireBlock - 1) / kWireBlock;
  const int64_t hdr = wire_header_bytes(nb);
  const char* p = payload + (int64_t)start * 64;
  const uint8_t* widths = (const uint8_t*)p + wire_align(4 * (int64_t)nb, 16);
  const uint8_t* q = (const uint8_t*)p + hdr;
  if (sg.kind != kWireI32) {
    const uint8_t flip = sg.kind == kWireI8 ? 0x80 : 0;
    for (int b = 0; b < nb; ++b) {
      const int cnt = std::min(kWireBlock, sg.n - b * kWireBlock);
      char* dst = sg.dst + (int64_t)b * kWireBlock;
      const uint8_t lo = (uint8_t)p[4 * b], hi = (uint8_t)p[4 * b + 1];
      if (widths[b]) std::memcpy(dst, q, (size_t)cnt), q += cnt;
      else if (sg.prev) clamp_block(dst, sg.prev + (int64_t)b * kWireBlock, cnt, lo ^ flip, hi ^ flip, flip);
      else std::memset(dst, lo, (size_t)cnt);
    }
    return wire_align(len, 64);
  }
  BiasWalk walk(sg.bias);
  for (int b = 0; b < nb; ++b) {
    const int cnt = std::min(kWireBlock, sg.n - b * kWireBlock);
    const int w = widths[b];
    int32_t base;
    std::memcpy(&base, p + 4 * b, 4);
    char* dst = sg.dst + 4 * (int64_t)b * kWireBlock;
    const char* prev = sg.prev ? sg.prev + 4 * (int64_t)b * kWireBlock : nullptr;
    if (sg.bias.addend && prev) {
      if (walk.run(cnt) == cnt) {  // one channel: the block's constant is its base plus that addend
        widen_w<true>(w, dst, prev, q, cnt, (uint32_t)base + walk.value());
        walk.advance(cnt);
      } else if (w == 0) {  // the prediction held: each channel run is its predecessor plus a constant
        for (int i = 0; i < cnt;) {
          const int k = walk.run(cnt - i);
          widen<0, true, false>(dst + 4 * i, prev + 4 * i, q, k, (uint32_t)base + walk.value(), nullptr);
          walk.advance(k);
          i += k;
        }
      } else {  // the constants of the block's channel runs, then one pass over the whole block
        uint32_t add[kWireBlock];
        for (int i = 0; i < cnt;) {
          const int k = walk.run(cnt - i);
          std::fill(add + i, add + i + k, (uint32_t)base + walk.value());
          walk.advance(k);
          i += k;
        }
        widen_w<true, true>(w, dst, prev, q, cnt, 0, add);
      }
    } else if (prev) {
      widen_w<true>(w, dst, prev, q, cnt, (uint32_t)base);
    } else {
      widen_w<false>(w, dst, nullptr, q, cnt, (uint32_t)base);
    }
    q += (int64_t)w * cnt;
  }
  return wire_align(len, 64);
}
}  // namespace

int wire_pool_threads() { return Pool::get().size(); }

int wire_decode(WireJob* job, int threads) {
  const auto t0 = std::chrono::steady_clock::now();
  job->status = 0;
  job->used_bytes = 0;
  const int64_t table = wire_table_bytes(job->n_seg);
  if (job->n_seg < 0 || !job->wire || job->wire_bytes < table) {
    job->status = TK_ERR_INVALID_ARG;
    return job->status;
  }
  std::atomic<int64_t> used{table};
  std::atomic<int> bad{0};
  const char* payload = job->wire + table;
  const int64_t payload_bytes = job->wire_bytes - table;
  Pool::get().run(job->n_units, threads, [&](int64_t u) {
    const WireUnit& un = job->units[u];
    int64_t sum = 0;
    for (int m = 0; m < un.count; ++m) {
      const int64_t r = decode_seg(*job, un.first + (int64_t)m * un.stride, payload, payload_bytes);
      if (r < 0) {
        bad.store(1, std::memory_order_relaxed);
        break;  // what follows in the chain would be added to undecoded bytes
      }
      sum += r;
    }
    used.fetch_add(sum, std::memory_order_relaxed);
  });
  job->used_bytes = used.load();
  job->status = bad.load() ? TK_ERR_INVALID_ARG : 0;
  job->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return job->status;
}

// ---------------------------------------------------------------- reference encoder
namespace {
// one segment at `out` (bias-coded where `walk` is given: it stands on the segment's first element);
// returns its unrounded length
int64_t encode_seg(const char* src, const char* prev, int n, char* out, BiasWalk* walk) {
  const int nb = (n + kWireBlock - 1) / kWireBlock;
  const int64_t hdr = wire_header_bytes(nb);
  std::memset(out, 0, (size_t)hdr);
  uint8_t* widths = (uint8_t*)out + wire_align(4 * (int64_t)nb, 16);
  uint8_t* q = (uint8_t*)out + hdr;
  for (int b = 0; b < nb; ++b) {
    const int cnt = std::min(kWireBlock, n - b * kWireBlock);
    int32_t v[kWireBlock];
    for (int i = 0; i < cnt; ++i) {
      uint32_t a, pv = 0;
      std::memcpy(&a, src + 4 * ((int64_t)b * kWireBlock + i), 4);
      if (prev) std::memcpy(&pv, prev + 4 * ((int64_t)b * kWireBlock + i), 4);
      v[i] = (int32_t)(a - pv);
    }
    if (walk)
      for (int i = 0; i < cnt;) {
        const int k = walk->run(cnt - i);
        for (int j = i; j < i + k; ++j) v[j] = (int32_t)((uint32_t)v[j] - walk->value());
        walk->advance(k);
        i += k;
      }
    const int32_t mn = *std::min_element(v, v + cnt), mx = *std::max_element(v, v + cnt);
    const uint32_t range = (uint32_t)mx - (uint32_t)mn;  // exact: mx >= mn as signed values
    const int w = range == 0 ? 0 : range <= 0xFFu ? 1 : range <= 0xFFFFu ? 2 : range <= 0xFFFFFFu ? 3 : 4;
    std::memcpy(out + 4 * b, &mn, 4);
    widths[b] = (uint8_t)w;
    for (int k = 0; k < w; ++k)
      for (int i = 0; i < cnt; ++i) q[k * cnt + i] = (uint8_t)(((uint32_t)v[i] - (uint32_t)mn) >> (8 * k));
    q += (int64_t)w * cnt;
  }
  return (char*)q - out;
}

// one segment of a 1-byte record (clamp-predicted from `prev` unless it is null)
int64_t encode_seg8(const char* src, const char* prev, int n, int kind, char* out) {
  const int nb = (n + kWireBlock - 1) / kWireBlock;
  const int64_t hdr = wire_header_bytes(nb);
  std::memset(out, 0, (size_t)hdr);
  uint8_t* widths = (uint8_t*)out + wire_align(4 * (int64_t)nb, 16);
  uint8_t* q = (uint8_t*)out + hdr;
  const uint8_t flip = kind == kWireI8 ? 0x80 : 0;
  for (int b = 0; b < nb; ++b) {
    const int cnt = std::min(kWireBlock, n - b * kWireBlock);
    const uint8_t* a = (const uint8_t*)src + (int64_t)b * kWireBlock;
    uint8_t lo = 0xFF, hi = 0;  // in the flipped (unsigned) order
    for (int i = 0; i < cnt; ++i) lo = std::min<uint8_t>(lo, a[i] ^ flip), hi = std::max<uint8_t>(hi, a[i] ^ flip);
    bool coded = lo == hi;
    if (prev && !coded) {
      const uint8_t* pv = (const uint8_t*)prev + (int64_t)b * kWireBlock;
      coded = true;
      for (int i = 0; i < cnt && coded; ++i) coded = clamp_u8((uint8_t)(pv[i] ^ flip), lo, hi) == (uint8_t)(a[i] ^ flip);
    }
    out[4 * b] = (char)(lo ^ flip), out[4 * b + 1] = (char)(hi ^ flip);
    widths[b] = coded ? 0 : 1;
    if (!coded) std::memcpy(q, a, (size_t)cnt), q += cnt;
  }
  return (char*)q - out;
}
}  // namespace
}  // namespace tk

extern "C" {

int64_t tk_wire_bound(const tk_wire_record* recs, int n_recs) {
  tk::WirePlan p;
  const int rc = tk::wire_plan(recs, n_recs, -1, "tk_wire_bound", &p, nullptr, true);
  return rc ? rc : p.bound;
}

int64_t tk_wire_encode_host(const tk_wire_record* recs, int n_recs, const void* image, int64_t image_bytes,
                            void* wire, int64_t wire_cap) {
  return tk_wire_encode_host_bias(recs, nullptr, n_recs, image, image_bytes, wire, wire_cap);
}

int64_t tk_wire_encode_host_bias(const tk_wire_record* recs, const tk_wire_addend* addends, int n_recs, const void* image,
                                 int64_t image_bytes, void* wire, int64_t wire_cap) {
  tk::WirePlan p;
  if (const int rc = tk::wire_plan(recs, n_recs, image_bytes, "tk_wire_encode_host", &p, addends)) return rc;
  if (!image || !wire || wire_cap < p.bound) {
    tk::set_error("tk_wire_encode_host: the wire buffer is smaller than tk_wire_bound");
    return TK_ERR_INVALID_ARG;
  }
  const int64_t table = tk::wire_table_bytes((int64_t)p.segs.size());
  std::memset(wire, 0, (size_t)table);
  char* payload = (char*)wire + table;
  int64_t cursor = 0;
  for (size_t i = 0; i < p.segs.size(); ++i) {
    const tk::WireSegRef& s = p.segs[i];
    const int kind = tk::wire_seg_kind(recs[s.rec].kind);
    const tk::WireSegAddr a =
        tk::wire_seg_addr(s, kind, (const char*)image + recs[s.rec].offset,
                          recs[s.rec].diff ? (const char*)image + recs[s.rec - 1].offset : nullptr);
    const uint32_t start = (uint32_t)(cursor / 64);
    std::memcpy((char*)wire + 4 * i, &start, 4);
    const tk::WireBias bias = tk::wire_seg_bias(recs, addends, s.rec, s.e0);
    tk::BiasWalk walk(bias);
    const int64_t len = kind == tk::kWireI32
                            ? tk::encode_seg(a.at, a.prev, s.n, payload + cursor, bias.addend ? &walk : nullptr)
                            : tk::encode_seg8(a.at, a.prev, s.n, kind, payload + cursor);
    const int64_t padded = tk::wire_align(len, 64);
    std::memset(payload + cursor + len, 0, (size_t)(padded - len));
    cursor += padded;
  }
  return table + cursor;
}

int tk_wire_decode(const tk_wire_record* recs, int n_recs, const void* wire, int64_t wire_bytes, void* image,
                   int64_t image_bytes, int threads) {
  return tk_wire_decode_bias(recs, nullptr, n_recs, wire, wire_bytes, image, image_bytes, threads);
}

int tk_wire_decode_bias(const tk_wire_record* recs, const tk_wire_addend* addends, int n_recs, const void* wire,
                        int64_t wire_bytes, void* image, int64_t image_bytes, int threads) {
  tk::WirePlan p;
  if (const int rc = tk::wire_plan(recs, n_recs, image_bytes, "tk_wire_decode", &p, addends)) return rc;
  if (!wire || !image || wire_bytes < 0) {
    tk::set_error("tk_wire_decode: null buffer");
    return TK_ERR_INVALID_ARG;
  }
  std::vector<tk::WireSegHost> segs(p.segs.size());
  for (size_t i = 0; i < p.segs.size(); ++i) {
    const tk::WireSegRef& s = p.segs[i];
    const tk::WireSegAddr a =
        tk::wire_seg_addr(s, recs[s.rec].kind, (char*)image + recs[s.rec].offset,
                          recs[s.rec].diff ? (const char*)image + recs[s.rec - 1].offset : nullptr);
    segs[i] = {a.at, a.prev, s.n, tk::wire_seg_kind(recs[s.rec].kind), tk::wire_seg_bias(recs, addends, s.rec, s.e0)};
  }
  tk::WireJob job{(const char*)wire, wire_bytes, segs.data(), (int64_t)segs.size(),
                  p.units.data(), (int64_t)p.units.size()};
  if (tk::wire_decode(&job, threads)) {
    tk::set_error("tk_wire_decode: the segment table or a segment does not lie inside the wire buffer");
    return TK_ERR_INVALID_ARG;
  }
  return TK_OK;
}

int tk_wire_check(const tk_wire_record* recs, int n_recs, const void* wire, int64_t wire_bytes) {
  return tk_wire_check_bias(recs, nullptr, n_recs, wire, wire_bytes);
}

// The addends are looked at as wire_plan looks at them (pointer, plane, channels): no value is read.
int tk_wire_check_bias(const tk_wire_record* recs, const tk_wire_addend* addends, int n_recs, const void* wire,
                       int64_t wire_bytes) {
  const char* who = addends ? "tk_wire_check_bias" : "tk_wire_check";  // errors name the entry point called
  tk::WirePlan p;
  if (const int rc = tk::wire_plan(recs, n_recs, -1, who, &p, addends)) return rc;
  const int64_t n_seg = (int64_t)p.segs.size();
  const int64_t table = tk::wire_table_bytes(n_seg);
  if (!wire || wire_bytes < table) {
    tk::set_error(who, "the segment table does not lie inside the wire buffer");
    return TK_ERR_INVALID_ARG;
  }
  const char* payload = (const char*)wire + table;
  for (int64_t i = 0; i < n_seg; ++i) {
    uint32_t start;
    std::memcpy(&start, (const char*)wire + 4 * i, 4);
    if (tk::wire_seg_extent(tk::wire_seg_kind(recs[p.segs[i].rec].kind), p.segs[i].n, start, payload,
                            wire_bytes - table) < 0) {
      tk::set_error(who, "segment " + std::to_string(i) + " (record " + std::to_string(p.segs[i].rec) +
                             ") does not lie inside the wire buffer or states a width its kind does not have");
      return TK_ERR_INVALID_ARG;
    }
  }
  return TK_OK;
}

int tk_wire_threads(void) { return tk::wire_pool_threads(); }

}  // extern "C"
