// pairwise_sum.h -- NumPy's pairwise summation as device code, shared by the kernels of
// fedagg.hip and scaffold16.hip (the numel == 1 patches).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fedagg_internal {

// ------------------------------------------------------------------------------------
// NumPy pairwise summation (loops_utils.h.src pairwise_sum, PW_BLOCKSIZE 128), on a
// generator get(i) of the n terms.  n <= 128: one leaf.
// ------------------------------------------------------------------------------------
template <typename T, typename G>
__device__ __forceinline__ T pw_leaf(const G& get, int64_t lo, int64_t n) {
#pragma clang fp contract(off)
  if (n < 8) {
    T res = T(-0.0);
    for (int64_t i = 0; i < n; ++i) res = res + get(lo + i);
    return res;
  }
  T r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = get(lo + j);
  int64_t i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = r[j] + get(lo + i + j);
  }
  T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res = res + get(lo + i);
  return res;
}

// Iterative form of the recursive split (n > 128: split at n/2 rounded down to a multiple of 8).
template <typename T, typename G>
__device__ T pw_sum(const G& get, int64_t n) {
#pragma clang fp contract(off)
  if (n <= 128) return pw_leaf<T>(get, 0, n);
  int64_t lo[64], nn[64];
  T left[64];
  int stage[64];
  int sp = 0;
  lo[0] = 0;
  nn[0] = n;
  stage[0] = 0;
  T ret = T(0);
  for (;;) {
    while (nn[sp] > 128) {  // descend into left halves
      int64_t n2 = nn[sp] / 2;
      n2 -= n2 % 8;
      stage[sp] = 1;
      lo[sp + 1] = lo[sp];
      nn[sp + 1] = n2;
      stage[sp + 1] = 0;
      ++sp;
    }
    ret = pw_leaf<T>(get, lo[sp], nn[sp]);
    bool done = true;
    while (sp > 0) {  // ascend: left done -> start right; right done -> combine
      --sp;
      if (stage[sp] == 1) {
        left[sp] = ret;
        stage[sp] = 2;
        int64_t n2 = nn[sp] / 2;
        n2 -= n2 % 8;
        lo[sp + 1] = lo[sp] + n2;
        nn[sp + 1] = nn[sp] - n2;
        stage[sp + 1] = 0;
        ++sp;
        done = false;
        break;
      }
      ret = left[sp] + ret;
    }
    if (done) return ret;
  }
}

}  // namespace fedagg_internal
