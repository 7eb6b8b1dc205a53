// The launch plan of libubresnet_sparse.so's compaction (ubz_compact of include/ubresnet_sparse.h) as plain C++: no HIP, so
// tests/sparse_host.cpp compiles it into a stand-alone program with the host sanitizers on.  The compaction is the pixel-block
// count / scan / rank of ubr_scan_plan.h with "lit" as the predicate; what is decided here is the grid cap of the fill and
// scatter launches, and host_count / host_write say what the count and write launches do with the shared walk.
#ifndef UBR_SPARSE_PLAN_H
#define UBR_SPARSE_PLAN_H

#include "ubr_scan_plan.h"

namespace ubz {

using namespace scanplan;                             // the constants, host_scan: under their names here as well
constexpr int MAX_GRID = 4096;                        // workgroups of the fill and scatter launches (they stride)

typedef scanplan::BlockPlan Plan;
inline bool make_plan(int64_t P, int64_t rows, int64_t cols, Plan* p) { return scanplan::make_block_plan(P, rows, cols, p); }
inline int64_t stride_grid(int64_t units) { return scanplan::stride_grid(units, LANES, MAX_GRID); }

// launch 1: scratch[b] = lit pixels of block b; launch 2 is scanplan::host_scan
inline void host_count(const Plan& p, const uint8_t* lit, uint32_t* scratch) {
  scanplan::host_count(p, [lit](int64_t q) { return lit[q] != 0; }, scratch);
}

// launch 3: the k-th lit pixel of the image goes to out_index[k], k < capacity; nothing at or past capacity is written
inline void host_write(const Plan& p, const uint8_t* lit, const uint32_t* scratch, int64_t capacity, int32_t* out_index) {
  scanplan::host_rank(p, [lit](int64_t q) { return lit[q] != 0; }, scratch, [=](int64_t q, int64_t k) {
    if (k < capacity) out_index[k] = (int32_t)q;
  });
}

}  // namespace ubz

#endif
