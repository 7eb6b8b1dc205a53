// The decision rule of libubresnet_stats.so (ubs_decide of include/ubresnet_stats.h) as inline functions that a host compiler
// takes as well: the kernel in ubr_stats.hip calls them on the device, tests/stats_host.cpp compiles them into a stand-alone
// program with the host sanitizers on.
#ifndef UBR_STATS_DECIDE_H
#define UBR_STATS_DECIDE_H

#include <stdint.h>
#include "../../include/ubresnet_stats.h"

#if defined(__HIPCC__)
#define UBS_HD __host__ __device__ __forceinline__
#else
#define UBS_HD inline
#endif

namespace ubs {

struct Verdict {
  int32_t keep;       // 1: commit (shadow <- live); 0: restore (live <- shadow)
  int32_t for_stats;  // 1: a restore that the optimizer's flag alone would not have caused
};

// has_flag 0: there is no optimizer flag (a NULL apply_flag), the step counts as applied; else it was applied iff flag != 0.
// check 0: bad rows never cause a restore.
UBS_HD Verdict decide(int32_t has_flag, int32_t flag, int32_t check, int32_t bad_rows) {
  const int32_t stepped = (has_flag == 0 || flag != 0) ? 1 : 0;
  const int32_t poisoned = (check != 0 && bad_rows > 0) ? 1 : 0;
  Verdict v;
  v.keep = (stepped != 0 && poisoned == 0) ? 1 : 0;
  v.for_stats = (stepped != 0 && poisoned != 0) ? 1 : 0;
  return v;
}

// the verdict into the control block: each counter moves once
UBS_HD void record(ubs_ctl* ctl, Verdict v, int32_t bad_rows) {
  ctl->keep = v.keep;
  ctl->bad_rows = bad_rows;
  if (v.keep != 0) {
    ctl->kept += 1;
  } else {
    ctl->restored += 1;
    if (v.for_stats != 0) ctl->restored_for_stats += 1;
  }
}

}  // namespace ubs

#endif
