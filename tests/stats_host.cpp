// The decision rule of libubresnet_stats.so (ubresnet_amd/csrc/ubr_stats_decide.h, plain C++ for a host compiler) as a
// stand-alone program, so that tests/test_cpu_stats.py can run it under the host sanitizers:
//   stats_host FLAG CHECK BAD_ROWS [FLAG CHECK BAD_ROWS ...]
// FLAG is `null` or an integer.  One control block, zeroed, takes the calls in order; after each the program prints one line
// `keep for_stats | keep bad_rows kept restored restored_for_stats` (the verdict, then the block's fields).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ubr_stats_decide.h"

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 1) % 3 != 0) {
    std::fprintf(stderr, "usage: %s FLAG CHECK BAD_ROWS [FLAG CHECK BAD_ROWS ...]\n", argv[0]);
    return 2;
  }
  ubs_ctl ctl;
  std::memset(&ctl, 0, sizeof ctl);
  for (int i = 1; i + 2 < argc; i += 3) {
    const bool has_flag = std::strcmp(argv[i], "null") != 0;
    const int32_t flag = has_flag ? (int32_t)std::atol(argv[i]) : 1;
    const int32_t check = (int32_t)std::atol(argv[i + 1]), bad_rows = (int32_t)std::atol(argv[i + 2]);
    const ubs::Verdict v = ubs::decide(has_flag ? 1 : 0, flag, check, bad_rows);
    ubs::record(&ctl, v, bad_rows);
    std::printf("%d %d | %d %d %lld %lld %lld\n", (int)v.keep, (int)v.for_stats, (int)ctl.keep, (int)ctl.bad_rows, (long long)ctl.kept,
                (long long)ctl.restored, (long long)ctl.restored_for_stats);
  }
  return 0;
}
