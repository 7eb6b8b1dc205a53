// The tile planner of libubresnet_group.so (ubresnet_amd/csrc/ubr_group_plan.h, plain C++) as a stand-alone program, so that
// tests/test_cpu_group.py can run it under the host sanitizers:
//   group_plan_host CAP UNIT0:UNITS [UNIT0:UNITS ...]
// plans the segments into a heap array of exactly CAP tiles (a write past it is the sanitizer's to report) and prints
//   count <tiles needed> err <PlanError> bad <segment at fault or -1>
// and then the tiles that were written, one `unit0 units seg` per line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ubr_group_plan.h"

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s CAP UNIT0:UNITS [UNIT0:UNITS ...]\n", argv[0]);
    return 2;
  }
  const long long cap = std::atoll(argv[1]);
  std::vector<int64_t> unit0, units;
  for (int i = 2; i < argc; ++i) {
    long long a = 0, b = 0;
    if (std::sscanf(argv[i], "%lld:%lld", &a, &b) != 2) {
      std::fprintf(stderr, "bad segment %s\n", argv[i]);
      return 2;
    }
    unit0.push_back(a);
    units.push_back(b);
  }
  ubg_tile* tiles = new ubg_tile[cap > 0 ? cap : 1];
  int err = 0;
  int64_t bad = -1;
  const int64_t nt = ubg::plan_tiles(unit0.data(), units.data(), (int64_t)unit0.size(), tiles, cap, &err, &bad);
  std::printf("count %lld err %d bad %lld\n", (long long)nt, err, (long long)bad);
  for (int64_t t = 0; t < nt && t < cap; ++t)
    std::printf("%lld %d %d\n", (long long)tiles[t].unit0, (int)tiles[t].units, (int)tiles[t].seg);
  delete[] tiles;
  return 0;
}
