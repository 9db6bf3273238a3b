// lib_error.h -- what every library next to libfedagg.so reports its errors with: the calling
// thread's error text (the library's *_last_error() returns it), fail() to set it from an
// argument check and check_launch() to set it from a refused kernel launch.
//
// One text per library and thread.  The namespace is hidden, so no library exports the text or the
// functions that write it: each .so that includes this header binds to its own copy at link time,
// however it is loaded (RTLD_GLOBAL included), and one library's text never shows in another's
// *_last_error().  Within a library the inline definitions are one object for all its sources.
#ifndef FEDAGG_LIB_ERROR_H
#define FEDAGG_LIB_ERROR_H

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

namespace fedagg_lib_error __attribute__((visibility("hidden"))) {

inline thread_local char g_error[256] = "";

__attribute__((format(printf, 2, 3))) inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
  return code;
}

// After a launch: OK, or EHIP with "<what>: <HIP's text>".  OK and EHIP are the including library's
// own codes; it binds them once, `constexpr auto check_launch = fedagg_lib_error::check_launch<...>;`.
template <int OK, int EHIP>
int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) return OK;
  snprintf(g_error, sizeof(g_error), "%s: %s", what, hipGetErrorString(e));
  return EHIP;
}

}  // namespace fedagg_lib_error

#endif  // FEDAGG_LIB_ERROR_H
