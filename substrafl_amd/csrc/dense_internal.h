// dense_internal.h -- what the sources of libfedagg_dense.so share: the blocking, the calling
// thread's error message and the argument checks every entry point makes before its first HIP call.
#ifndef FEDAGG_DENSE_INTERNAL_H
#define FEDAGG_DENSE_INTERNAL_H

#include <hip/hip_runtime.h>

#include <cstdio>

#include "fedagg_dense.h"

#define DN_NB 32      // panel width; block of the triangular solves and substitutions
#define DN_TM 64      // trailing-update tile, rows
#define DN_TN 64      // trailing-update tile, columns
#define DN_BLOCK 256
#define DN_LS (DN_NB + 4)  // LDS row stride of a tile's 32 k-values: 4 (mod 32) doubles, the 64 operand reads 2 per bank

typedef double dn_f64x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long dn_u64;

namespace fedagg_dense_detail {

inline thread_local char g_error[256] = "";  // one per thread for the whole library (fedagg_dense_last_error)

inline int fail(int code, const char* fmt, long long v = 0) {
  snprintf(g_error, sizeof(g_error), fmt, v);
  return code;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) return FEDAGG_DENSE_OK;
  snprintf(g_error, sizeof(g_error), "%s: %s", what, hipGetErrorString(e));
  return FEDAGG_DENSE_EHIP;
}

// The argument checks every entry point shares (n >= 1 here), before any HIP call.
inline int check_matrix(const void* d_A, uint64_t n, uint64_t lda) {
  if (!d_A) return fail(FEDAGG_DENSE_EINVAL, "d_A is NULL");
  if (n > FEDAGG_DENSE_MAX_N) return fail(FEDAGG_DENSE_EINVAL, "n = %lld exceeds FEDAGG_DENSE_MAX_N", (long long)n);
  if (lda < n) return fail(FEDAGG_DENSE_EINVAL, "lda = %lld is smaller than n", (long long)lda);
  if (lda > UINT64_MAX / 8 / n) return fail(FEDAGG_DENSE_EINVAL, "n * lda * 8 overflows 64 bits (n = %lld)", (long long)n);
  return FEDAGG_DENSE_OK;
}

inline unsigned blocks_for(dn_u64 work) { return (unsigned)((work + DN_BLOCK - 1) / DN_BLOCK); }

}  // namespace fedagg_dense_detail

#endif  // FEDAGG_DENSE_INTERNAL_H
