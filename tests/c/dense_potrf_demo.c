/* The dense Cholesky from plain C (no HIP headers, no Python): A = L L^T for the integer factor
 * L = [2 0 0; 1 1 0; -2 1 4], staged and fetched through the native session of fedagg.h, factored
 * by fedagg_dense_potrf_f64 on the session stream.  Every intermediate is a small integer, so L
 * comes back to the last bit; the strict upper triangle holds a marker the call must leave alone.
 * A second matrix, the same with a_11 lowered by l_11^2, stops at pivot 2 (info = 2).
 * Build: gcc -O2 -Iinclude tests/c/dense_potrf_demo.c -Lsubstrafl_amd -lfedagg_dense -lfedagg */
#include <stdint.h>
#include <stdio.h>

#include "fedagg.h"
#include "fedagg_dense.h"

#define N 3
#define MARK -99.0

static int factor(fedagg_session* s, double* a, int32_t* info) {
  void *d_a = NULL, *d_i = NULL;
  const void* seg[1] = {a};
  uint64_t bytes[1] = {N * N * sizeof(double)};
  if (fedagg_session_buffer(s, 0, bytes[0], &d_a) || fedagg_session_buffer(s, 1, sizeof(*info), &d_i) ||
      fedagg_session_stage(s, d_a, bytes[0], 1, 1, seg, bytes)) {
    fprintf(stderr, "session: %s\n", fedagg_last_error());
    return 2;
  }
  if (fedagg_dense_potrf_f64((double*)d_a, N, N, (int32_t*)d_i, fedagg_session_stream(s))) {
    fprintf(stderr, "potrf: %s\n", fedagg_dense_last_error());
    return 2;
  }
  if (fedagg_session_fetch(s, d_a, a, bytes[0]) || fedagg_session_fetch(s, d_i, info, sizeof(*info))) {
    fprintf(stderr, "fetch: %s\n", fedagg_last_error());
    return 2;
  }
  return 0;
}

int main(void) {
  /* row-major, the lower triangle of L L^T */
  double a[N * N] = {4.0, MARK, MARK, 2.0, 2.0, MARK, -4.0, -1.0, 21.0};
  double b[N * N] = {4.0, MARK, MARK, 2.0, 1.0, MARK, -4.0, -1.0, 21.0};
  const double want[N * N] = {2.0, MARK, MARK, 1.0, 1.0, MARK, -2.0, 1.0, 4.0};
  int32_t info_a = -1, info_b = -1;
  fedagg_session* s = fedagg_session_create(0);
  if (!s) {
    fprintf(stderr, "session: %s\n", fedagg_last_error());
    return 2;
  }
  if (factor(s, a, &info_a) || factor(s, b, &info_b)) return 2;
  fedagg_session_destroy(s);
  int bad = (info_a != 0) + (info_b != 2) + (b[0] != 2.0);
  for (int i = 0; i < N * N; ++i) bad += a[i] != want[i];
  printf("dense_potrf_demo: L = [%g; %g %g; %g %g %g] info = %d, then info = %d (abi %d)\n", a[0], a[3], a[4], a[6],
         a[7], a[8], (int)info_a, (int)info_b, fedagg_dense_abi_version());
  return bad ? 1 : 0;
}
