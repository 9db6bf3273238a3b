/* The dense Householder LQ from plain C (no HIP headers, no Python): a 3 x 5 row-major matrix
 * staged and fetched through the native session of fedagg.h, factored by fedagg_dense_gelqf_f64,
 * Q formed by fedagg_dense_orglq_f64 on the session stream.  Prints ||Q Q^T - I||_F and
 * ||A - L Q||_F; both must be a few units of 2^-53.
 * Build: gcc -O2 -Iinclude tests/c/dense_lq_demo.c -Lsubstrafl_amd -lfedagg_dense -lfedagg -lm */
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "fedagg.h"
#include "fedagg_dense.h"

#define N 3
#define M 5

int main(void) {
  const double a[N * M] = {2.0, -1.0, 0.5, 3.0, 1.0, 1.0, 4.0, -2.0, 0.25, 1.5, -3.0, 1.0, 1.0, 2.0, -0.5};
  double f[N * M], q[N * M], tau[N];
  void *d_a = NULL, *d_q = NULL, *d_tau = NULL, *d_ws = NULL;
  const void* seg[1] = {a};
  uint64_t bytes[1] = {sizeof(a)};
  int panel, tile_m, tile_n, k_chunk;
  fedagg_session* s = fedagg_session_create(0);
  if (!s) {
    fprintf(stderr, "session: %s\n", fedagg_last_error());
    return 2;
  }
  if (fedagg_dense_lq_blocking(&panel, &tile_m, &tile_n, &k_chunk)) return 2;
  if (fedagg_session_buffer(s, 0, sizeof(a), &d_a) || fedagg_session_buffer(s, 1, sizeof(q), &d_q) ||
      fedagg_session_buffer(s, 2, sizeof(tau), &d_tau) ||
      fedagg_session_buffer(s, 3, fedagg_dense_lq_ws_bytes(N, M), &d_ws) ||
      fedagg_session_stage(s, d_a, bytes[0], 1, 1, seg, bytes)) {
    fprintf(stderr, "session: %s\n", fedagg_last_error());
    return 2;
  }
  if (fedagg_dense_gelqf_f64((double*)d_a, N, M, M, (double*)d_tau, d_ws, fedagg_session_stream(s)) ||
      fedagg_dense_orglq_f64((const double*)d_a, N, M, M, (const double*)d_tau, (double*)d_q, M, d_ws,
                             fedagg_session_stream(s))) {
    fprintf(stderr, "lq: %s\n", fedagg_dense_last_error());
    return 2;
  }
  if (fedagg_session_fetch(s, d_a, f, sizeof(f)) || fedagg_session_fetch(s, d_q, q, sizeof(q)) ||
      fedagg_session_fetch(s, d_tau, tau, sizeof(tau))) {
    fprintf(stderr, "fetch: %s\n", fedagg_last_error());
    return 2;
  }
  fedagg_session_destroy(s);
  double orth = 0.0, res = 0.0;
  for (int i = 0; i < N; ++i)
    for (int k = 0; k < N; ++k) {
      double g = i == k ? -1.0 : 0.0;
      for (int c = 0; c < M; ++c) g += q[i * M + c] * q[k * M + c];
      orth += g * g;
    }
  for (int i = 0; i < N; ++i)
    for (int c = 0; c < M; ++c) {
      double r = a[i * M + c];
      for (int k = 0; k <= i; ++k) r -= f[i * M + k] * q[k * M + c]; /* L: on and below the diagonal */
      res += r * r;
    }
  orth = sqrt(orth);
  res = sqrt(res);
  printf("dense_lq_demo: %d x %d, blocking %d/%d/%d/%d, tau = [%g %g %g], ||Q Q^T - I|| = %.3g, ||A - L Q|| = %.3g (abi %d)\n",
         N, M, panel, tile_m, tile_n, k_chunk, tau[0], tau[1], tau[2], orth, res, fedagg_dense_abi_version());
  return (orth < 1e-14 && res < 1e-13) ? 0 : 1;
}
