// Stand-alone check of the float statistics' host side (tk::fstats_layout, csrc/tk_fstats.hip) for
// sanitizer builds: the job table a plan uploads -- which records get a job, their first
// workgroups, the span of a record of more than kFStatsMaxGroups spans -- and every refusal, on
// buffer addresses that are never dereferenced.  CPU only; launches nothing and never needs a
// device.
//
//   hipcc -std=c++20 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=all -I include tools/fstats_table_check.cc \
//       tachikoma_amd/csrc/tk_fstats.hip -o fstats_table_check && ./fstats_table_check
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../tachikoma_amd/csrc/tk_fstats.h"

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

int main() {
  const int64_t S = tk::kFStatsSpan;
  std::vector<tk::FStatsJob> jobs;
  int64_t blocks = -1;
  // one workgroup, none, exactly one span, one element more, a misaligned-by-4 buffer, 513 spans
  const void* src[6] = {(void*)0x1000, nullptr, (void*)0x100000, (void*)0x900000, (void*)0x1100004, (void*)0x2000000};
  const int64_t n[6] = {1, 0, S, S + 1, 2 * S + 17, 513 * S};
  CHECK(tk::fstats_layout(src, n, 6, "check", &jobs, &blocks) == TK_OK);
  CHECK(jobs.size() == 5 && blocks == 1 + 1 + 2 + 3 + 257);
  if (jobs.size() == 5) {
    const int rec[5] = {0, 2, 3, 4, 5};
    const int64_t first[5] = {0, 1, 2, 4, 7};
    for (int i = 0; i < 5; ++i) {
      CHECK(jobs[i].rec == rec[i] && jobs[i].first_blk == first[i] && jobs[i].n == n[rec[i]]);
      CHECK((const void*)jobs[i].src == src[rec[i]]);
      CHECK(jobs[i].span == (i == 4 ? 2 * S : S));
      // the workgroups of a record cover it exactly: the last one starts inside it
      const int64_t groups = (i == 4 ? blocks : first[i + 1]) - first[i];
      CHECK((groups - 1) * jobs[i].span < jobs[i].n && groups * jobs[i].span >= jobs[i].n);
      CHECK(groups <= tk::kFStatsMaxGroups);
    }
  }
  // records of no elements only: a plan without workgroups
  const int64_t none[2] = {0, 0};
  CHECK(tk::fstats_layout(src, none, 2, "check", &jobs, &blocks) == TK_OK && jobs.empty() && blocks == 0);
  // the largest record the table takes: 2^40 elements in kFStatsMaxGroups workgroups
  const int64_t huge[1] = {(int64_t)1 << 40};
  CHECK(tk::fstats_layout(src, huge, 1, "check", &jobs, &blocks) == TK_OK && jobs.size() == 1);
  CHECK(blocks == tk::kFStatsMaxGroups && jobs[0].span * blocks == huge[0]);

  // refusals leave the table alone
  jobs.assign(3, tk::FStatsJob{});
  blocks = 77;
  auto refused = [&](const void* const* s, const int64_t* cnt, int count, const char* word) {
    tk::g_err.clear();
    CHECK(tk::fstats_layout(s, cnt, count, "check", &jobs, &blocks) == TK_ERR_INVALID_ARG);
    CHECK(jobs.size() == 3 && blocks == 77);
    CHECK(tk::g_err.find(word) != std::string::npos && tk::g_err.rfind("check: ", 0) == 0);
  };
  refused(nullptr, n, 6, "null");
  refused(src, nullptr, 6, "null");
  refused(src, n, 0, "no records");
  refused(src, n, -3, "no records");
  const int64_t negative[2] = {5, -1};
  refused(src, negative, 2, "record 1");
  const int64_t too_many[1] = {((int64_t)1 << 40) + 1};
  refused(src, too_many, 1, "element count");
  const void* odd[2] = {(void*)0x1000, (void*)0x2002};
  const int64_t two[2] = {4, 4};
  refused(odd, two, 2, "4-byte");
  const void* null_buf[1] = {nullptr};
  refused(null_buf, two, 1, "null buffer");
  CHECK(tk::fstats_layout(src, n, 6, "check", nullptr, &blocks) == TK_ERR_INVALID_ARG);
  CHECK(tk::fstats_layout(src, n, 6, "check", &jobs, nullptr) == TK_ERR_INVALID_ARG);
  std::printf(g_fail ? "fstats_table_check: %d failures\n" : "fstats_table_check: ok\n", g_fail);
  return g_fail ? 1 : 0;
}
