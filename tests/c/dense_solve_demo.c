/* The dense solve from plain C (no HIP headers, no Python): a 3 x 3 system whose first pivot
 * must be taken from the last row, staged and fetched through the native session of fedagg.h,
 * solved by fedagg_dense_solve_f64 on the session stream.  The numbers are small integers, so
 * the factorisation is exact and x = (1, 2, 3) comes back to the last bit.
 * Build: gcc -O2 -Iinclude tests/c/dense_solve_demo.c -Lsubstrafl_amd -lfedagg_dense -lfedagg */
#include <stdint.h>
#include <stdio.h>

#include "fedagg.h"
#include "fedagg_dense.h"

#define N 3

int main(void) {
  /* row-major; b = A (1, 2, 3)^T */
  double a[N * N] = {0.0, 2.0, 1.0, 1.0, 1.0, 0.0, 4.0, 0.0, 2.0};
  double b[N] = {7.0, 3.0, 10.0};
  int32_t ints[N + 1]; /* ipiv, then info */
  int panel = 0, tile_m = 0, tile_n = 0;
  if (fedagg_dense_blocking(&panel, &tile_m, &tile_n) || panel <= 0) {
    fprintf(stderr, "blocking: %s\n", fedagg_dense_last_error());
    return 2;
  }
  fedagg_session* s = fedagg_session_create(0);
  if (!s) {
    fprintf(stderr, "session: %s\n", fedagg_last_error());
    return 2;
  }
  void *d_a = NULL, *d_b = NULL, *d_i = NULL, *d_ws = NULL;
  const uint64_t ws = fedagg_dense_ws_bytes(N);
  if (fedagg_session_buffer(s, 0, sizeof(a), &d_a) || fedagg_session_buffer(s, 1, sizeof(b), &d_b) ||
      fedagg_session_buffer(s, 2, sizeof(ints), &d_i) || (ws && fedagg_session_buffer(s, 3, ws, &d_ws))) {
    fprintf(stderr, "buffer: %s\n", fedagg_last_error());
    return 2;
  }
  const void* seg_a[1] = {a};
  const void* seg_b[1] = {b};
  uint64_t bytes_a[1] = {sizeof(a)}, bytes_b[1] = {sizeof(b)};
  if (fedagg_session_stage(s, d_a, sizeof(a), 1, 1, seg_a, bytes_a) ||
      fedagg_session_stage(s, d_b, sizeof(b), 1, 1, seg_b, bytes_b)) {
    fprintf(stderr, "stage: %s\n", fedagg_last_error());
    return 2;
  }
  if (fedagg_dense_solve_f64((double*)d_a, N, N, (int32_t*)d_i, (int32_t*)d_i + N, (double*)d_b, d_ws,
                             fedagg_session_stream(s))) {
    fprintf(stderr, "solve: %s\n", fedagg_dense_last_error());
    return 2;
  }
  if (fedagg_session_fetch(s, d_b, b, sizeof(b)) || fedagg_session_fetch(s, d_i, ints, sizeof(ints))) {
    fprintf(stderr, "fetch: %s\n", fedagg_last_error());
    return 2;
  }
  fedagg_session_destroy(s);
  const int bad = (b[0] != 1.0) + (b[1] != 2.0) + (b[2] != 3.0) + (ints[N] != 0) + (ints[0] != 2);
  printf("dense_solve_demo: x = (%g, %g, %g) ipiv0 = %d info = %d blocking %d/%d/%d (abi %d)\n", b[0], b[1], b[2],
         (int)ints[0], (int)ints[N], panel, tile_m, tile_n, fedagg_dense_abi_version());
  return bad ? 1 : 0;
}
