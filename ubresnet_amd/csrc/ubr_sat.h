// What every satellite library (one .hip file behind one public header of include/) needs on the host side: the error message
// of the calling thread, the two check macros that fill it and return, the alignment and overlap predicates of the argument
// checks, and the library's two exports <prefix>_last_error and <prefix>_version.  Everything here has internal linkage: the
// libraries link against none of the others, each has a copy of its own.  No other header of the project is included here, and
// the network's library (ubr_common.h, ubr_host.h) does not include this one.
#ifndef UBR_SAT_H
#define UBR_SAT_H

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

namespace sat {

static thread_local char g_err[512] = "";

static void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

inline bool aligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; }     // `to` a power of two
inline bool aligned16(const void* p) { return aligned(p, 16); }

// two byte ranges share a byte; a null pointer overlaps nothing
inline bool overlap(const void* a, unsigned long long abytes, const void* b, unsigned long long bbytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x != 0 && y != 0 && x < y + bbytes && y < x + abytes;
}

}  // namespace sat

// The return values are every public header's UBx_EINVAL and UBx_ELAUNCH; SAT_RETURN_CODES(UBx) in a source holds them to it.
#define SAT_RETURN_CODES(P) \
  static_assert(P##_OK == 0 && P##_EINVAL == -1 && P##_ELAUNCH == -2, "the shared return values are those of the public header")

#define SAT_CHECK(cond, ...)          \
  do {                                \
    if (!(cond)) {                    \
      sat::set_error(__VA_ARGS__);    \
      return -1;                      \
    }                                 \
  } while (0)

#define SAT_LAUNCH_CHECK(name)                                                       \
  do {                                                                               \
    hipError_t e_ = hipGetLastError();                                               \
    if (e_ != hipSuccess) {                                                          \
      sat::set_error("%s: launch failed: %s", (name), hipGetErrorString(e_));        \
      return -2;                                                                     \
    }                                                                                \
  } while (0)

#define SAT_EXPORTS(prefix, version)                                          \
  extern "C" const char* prefix##_last_error(void) { return sat::g_err; }     \
  extern "C" int prefix##_version(void) { return (version); }

#endif
