// The guarded optimizer's rule (ubresnet_amd/csrc/ubr_opt_rule.h, plain C++ for a host compiler) as a stand-alone program, so
// that tests/test_cpu_opt.py can run it under the host sanitizers:
//   opt_rule_host
// It prints one line per case; every fp32 number is a 32-bit pattern in hexadecimal, every fp64 number a 64-bit one:
//   T i | bc1 sqrt_bc2                                                       row i of the program's bias-correction table
//   Q acc x y z w | acc'                                                     optrule::sumsq4
//   D sumsq grad_scale max_norm skip bc_len | norm scale gscale apply clipped bc1 sqrt_bc2 applied skipped clipped_total row0..3
//                                                                            decide + record + bc_row on one ubo_ctl, in sequence
//   A p g m v gscale wd b1 b2 eps lr t bc_len | p' m' v'                     bc_row + optrule::adam_element
//   S p g b gscale wd lr momentum dampening has_buf first nesterov | p' b'   optrule::sgd_element
// The decision is recorded in a ubg_ctl as well; the program fails if the two heads ever differ in a byte.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../include/ubresnet_group.h"
#include "../../include/ubresnet_opt.h"
#include "ubr_opt_rule.h"

static float f32(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
static double f64(uint64_t b) { double d; std::memcpy(&d, &b, 8); return d; }
static unsigned long long bits(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }

// rows 1 .. 4 of the table of beta1 = 0.9, beta2 = 0.999 (bc1, sqrt_bc2)
static const uint32_t kTable[4][2] = {{0x3dccccd0u, 0x3d0186acu}, {0x3e428f5fu, 0x3d3721b8u}, {0x3e8ac085u, 0x3d603bcau},
                                      {0x3eb013abu, 0x3d816dcfu}};

int main() {
  static_assert(sizeof(ubo_ctl) == sizeof(ubg_ctl), "the two heads have one layout");
  float table[8];
  for (int i = 0; i < 4; ++i) {
    table[2 * i] = f32(kTable[i][0]);
    table[2 * i + 1] = f32(kTable[i][1]);
    std::printf("T %d | %08x %08x\n", i, kTable[i][0], kTable[i][1]);
  }

  const double accs[] = {0.0, 1.0, 0x1p-60, 1e300};
  const uint32_t xs[][4] = {{0x3f800000u, 0x40000000u, 0x40400000u, 0x40800000u}, {0x3dcccccdu, 0xbf19999au, 0x00000001u, 0x7f7fffffu},
                            {0x00000000u, 0x80000000u, 0x7f800000u, 0x3f800000u}, {0x7fc00000u, 0x3f800000u, 0x3f800000u, 0x3f800000u}};
  for (double acc : accs)
    for (const auto& x : xs)
      std::printf("Q %016llx %08x %08x %08x %08x | %016llx\n", bits(acc), x[0], x[1], x[2], x[3],
                  bits(optrule::sumsq4(acc, f32(x[0]), f32(x[1]), f32(x[2]), f32(x[3]))));

  // the decisions of one control block, in sequence: not clipped; clipped (with a negative grad_scale); max_norm < 0; a sum of 0,
  // inf and NaN, each with the guard on and off; max_norm 0; then a table shorter than the applied count
  struct Case { uint64_t sumsq; uint32_t grad_scale, max_norm; int skip; long bc_len; };
  const uint64_t INF = 0x7ff0000000000000ull, NAN_ = 0x7ff8000000000000ull, NINE = 0x4022000000000000ull, SIXTEEN = 0x4030000000000000ull,
                 FOUR = 0x4010000000000000ull, THIRD = 0x3fd5555555555555ull;
  const uint32_t ONE = 0x3f800000u, SIX = 0x40c00000u, MHALF = 0xbf000000u, MONE = 0xbf800000u, ZERO = 0u, S1024 = 0x44800000u;
  const Case cases[] = {{NINE, ONE, SIX, 1, 4}, {SIXTEEN, MHALF, ONE, 1, 4}, {FOUR, ONE, MONE, 1, 4},
                        {0ull, ONE, ONE, 1, 4}, {0ull, ONE, ONE, 0, 4}, {INF, ONE, ONE, 1, 4}, {INF, ONE, ONE, 0, 4},
                        {NAN_, ONE, ONE, 1, 4}, {NAN_, ONE, ONE, 0, 4}, {NAN_, ONE, MONE, 0, 4}, {NINE, ONE, ZERO, 1, 4},
                        {THIRD, S1024, 0x3dcccccdu, 1, 2}, {NINE, ONE, SIX, 1, 1}, {THIRD, 0x3a83126fu, 0x3a83126fu, 0, 3}};
  ubo_ctl o;
  ubg_ctl g;
  std::memset(&o, 0, sizeof(o));
  std::memset(&g, 0, sizeof(g));
  for (const Case& c : cases) {
    const double sumsq = f64(c.sumsq);
    const optrule::Decision d = optrule::decide(sumsq, f32(c.grad_scale), f32(c.max_norm), c.skip);
    optrule::record(o, sumsq, d);
    optrule::record(g, sumsq, d);
    if (d.apply) {
      optrule::bc_row(table, c.bc_len, o.applied, o.bc1, o.sqrt_bc2);
      g.bc1 = o.bc1;                                                  // (the group's head leaves them to its segments)
      g.sqrt_bc2 = o.sqrt_bc2;
    }
    if (std::memcmp(&o, &g, sizeof(o)) != 0 || bits(o.sumsq) != c.sumsq) {
      std::fprintf(stderr, "the heads of ubo_ctl and ubg_ctl differ\n");
      return 1;
    }
    std::printf("D %016llx %08x %08x %d %ld | %08x %08x %08x %d %d %08x %08x %lld %lld %lld %08x %08x %08x %08x\n",
                (unsigned long long)c.sumsq, c.grad_scale, c.max_norm, c.skip, c.bc_len, bits(o.norm), bits(o.scale), bits(o.gscale), o.apply,
                o.clipped, bits(o.bc1), bits(o.sqrt_bc2), (long long)o.applied, (long long)o.skipped, (long long)o.clipped_total,
                bits(o.row[0]), bits(o.row[1]), bits(o.row[2]), bits(o.row[3]));
  }

  // elements: ordinary values whose products are not representable, so that a second rounding of the fused multiply-add shows
  const uint32_t P[] = {0x3f9e0419u, 0xbdcccccdu, 0x4048f5c3u}, G[] = {0x3e99999au, 0xbf2aaaabu, 0x3c23d70au};
  const uint32_t M[] = {0x00000000u, 0x3d4ccccdu, 0xbe19999au}, V[] = {0x00000000u, 0x3a83126fu, 0x3dcccccdu};
  const uint32_t GS[] = {0x3f800000u, 0x3eaaaaabu}, WD[] = {0x00000000u, 0x38d1b717u, 0x3dcccccdu};
  const uint32_t B1 = 0x3f666666u, B2 = 0x3f7fbe77u, EPS = 0x322bcc77u, LR = 0x3a83126fu;
  const long long ts[] = {1, 3, 9};                                   // the first row, one inside, one past the table's end
  for (long long t : ts)
    for (int i = 0; i < 3; ++i)
      for (uint32_t gs : GS)
        for (uint32_t wd : WD) {
          float p = f32(P[i]), m = f32(M[i]), v = f32(V[i]), bc1, sqrt_bc2;
          optrule::bc_row(table, 4, t, bc1, sqrt_bc2);
          optrule::adam_element(p, f32(G[i]), m, v, f32(gs), f32(wd), f32(B1), f32(B2), f32(EPS), f32(LR) / bc1, sqrt_bc2);
          std::printf("A %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %lld 4 | %08x %08x %08x\n", P[i], G[i], M[i], V[i], gs, wd, B1, B2,
                      EPS, LR, t, bits(p), bits(m), bits(v));
        }
  // SGD: plain (no buffer); momentum, first and later step; nesterov, first and later step; with and without dampening
  const uint32_t MOM = 0x3f666666u, DAMP[] = {0x00000000u, 0x3dcccccdu}, LR2 = 0x3c23d70au;
  struct Form { int has_buf, first, nesterov; };
  const Form forms[] = {{0, 0, 0}, {0, 1, 0}, {1, 1, 0}, {1, 0, 0}, {1, 1, 1}, {1, 0, 1}};
  for (const Form& f : forms)
    for (int i = 0; i < 3; ++i)
      for (uint32_t gs : GS)
        for (uint32_t wd : WD)
          for (uint32_t damp : DAMP) {
            const uint32_t mom = f.has_buf ? MOM : 0u;
            float p = f32(P[i]), b = f32(M[i]);
            optrule::sgd_element(p, f32(G[i]), b, f32(gs), f32(wd), f32(LR2), f32(mom), f32(damp), f.has_buf != 0, f.first, f.nesterov);
            std::printf("S %08x %08x %08x %08x %08x %08x %08x %08x %d %d %d | %08x %08x\n", P[i], G[i], M[i], gs, wd, LR2, mom, damp, f.has_buf,
                        f.first, f.nesterov, bits(p), bits(b));
          }
  return 0;
}
