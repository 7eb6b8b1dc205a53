// The tile planner of libubresnet_group.so (ubg_plan_tiles of include/ubresnet_group.h) as plain C++: no HIP, so
// tests/group_plan_host.cpp compiles it into a stand-alone program with the host sanitizers on.
#ifndef UBR_GROUP_PLAN_H
#define UBR_GROUP_PLAN_H

#include <stdint.h>
#include "../../include/ubresnet_group.h"

namespace ubg {

enum PlanError { PLAN_OK = 0, PLAN_NULL = 1, PLAN_NSEG = 2, PLAN_UNITS = 3, PLAN_ORDER = 4, PLAN_CAP = 5 };

// -> number of tiles the segments need, written to tiles[0 .. min(that, cap)); *err says why a plan is refused and *bad which
// segment is at fault.  Nothing is written at or past tiles[cap].
inline int64_t plan_tiles(const int64_t* seg_unit0, const int64_t* seg_units, int64_t nseg, ubg_tile* tiles, int64_t cap,
                          int* err, int64_t* bad) {
  *err = PLAN_OK;
  *bad = -1;
  if (seg_unit0 == nullptr || seg_units == nullptr || tiles == nullptr) { *err = PLAN_NULL; return 0; }
  if (nseg < 1 || nseg > INT32_MAX) { *err = PLAN_NSEG; return 0; }
  int64_t end = 0;
  for (int64_t s = 0; s < nseg; ++s) {          // all of the input is checked before anything is written
    *bad = s;
    if (seg_units[s] < 1 || seg_units[s] > (INT64_MAX >> 4)) { *err = PLAN_UNITS; return 0; }
    if (seg_unit0[s] < end || seg_unit0[s] > (INT64_MAX >> 4)) { *err = PLAN_ORDER; return 0; }
    end = seg_unit0[s] + seg_units[s];
  }
  *bad = -1;
  int64_t nt = 0;
  for (int64_t s = 0; s < nseg; ++s) {
    const int64_t cnt = (seg_units[s] + UBG_TILE_UNITS - 1) / UBG_TILE_UNITS;
    for (int64_t k = 0; k < cnt && nt + k < cap; ++k) {      // tiles past `cap` are counted, not written
      const int64_t left = seg_units[s] - k * UBG_TILE_UNITS;
      tiles[nt + k].unit0 = seg_unit0[s] + k * UBG_TILE_UNITS;
      tiles[nt + k].units = (int32_t)(left < UBG_TILE_UNITS ? left : UBG_TILE_UNITS);
      tiles[nt + k].seg = (int32_t)s;
    }
    nt += cnt;
  }
  if (nt > cap) *err = PLAN_CAP;
  return nt;
}

}  // namespace ubg

#endif
