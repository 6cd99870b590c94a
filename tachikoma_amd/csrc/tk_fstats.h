// Float statistics (tk_fstats.hip): the job table of a plan over float32 records.  Shared by the
// kernel file and by the stand-alone check of the table's layout (tools/fstats_table_check.cc).
#pragma once

#include <string>
#include <vector>

#include "tk_common.h"

namespace tk {

constexpr int kFStatsTile = 1024;   // elements of one tile: 256 lanes x 16 bytes
constexpr int kFStatsTiles = 128;   // tiles a workgroup walks before it flushes
constexpr int64_t kFStatsSpan = (int64_t)kFStatsTile * kFStatsTiles;  // 512 KiB of a record
constexpr int kFStatsMaxGroups = 512;  // workgroups of one record: a larger record gets longer spans
constexpr int kFStatsMinBins = 2, kFStatsMaxBins = 8192;
constexpr int kFStatsDigits = 2048;    // entries of a record's digit table (levels 1, 2: the first 1024)

struct FStatsJob {
  const float* src;
  int64_t n;          // elements, > 0
  int64_t first_blk;  // first workgroup of the record
  int64_t span;       // elements per workgroup: a whole number of kFStatsSpan
  int32_t rec;        // entry of the result arrays
  int32_t pad;
};

// Validates n records under the entry point's name `who` and lays their jobs out: records of no
// elements get no job, workgroups are numbered from 0, *blocks is their number.  Host only; on a
// refusal `jobs` and `blocks` are left alone.
int fstats_layout(const void* const* src, const int64_t* n_elems, int n, const char* who, std::vector<FStatsJob>* jobs,
                  int64_t* blocks);

}  // namespace tk
