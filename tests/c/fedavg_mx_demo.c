/* FedAvg over MXFP8 client rows from plain C (no HIP headers, no Python): the K code rows and the K
 * scale rows staged as two byte buckets through the session of libfedagg.so, one
 * fedagg_mx_fedavg_e4m3 call of libfedagg_mx.so, the fp32 result fetched, against the reference
 * order on the host (fed_avg.py:217-222 on the decoded rows: x = v * 2^(s-127) by ldexpf, exact;
 * acc = +0.0; acc = fl(acc + fl(x_k * w_k)), all in float), bit for bit.  M is no multiple of 16 or
 * 32 and covers two workgroup steps and a tail; two numel == 1 indices (K < 8, so NumPy's pairwise
 * order over the K products is the plain one and the host loop covers them too: no code here is
 * a zero or a NaN).
 * Usage: fedavg_mx_demo [device]
 * Build: gcc -O2 -ffp-contract=off -Iinclude tests/c/fedavg_mx_demo.c -Lsubstrafl_amd -lfedagg_mx -lfedagg -lm */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fedagg_mx.h"

#define K 5
#define M 8215u /* 2 x 4096 + 23 */

static uint32_t lcg(uint32_t* s) { return *s = *s * 1664525u + 1013904223u; }

static float decode(uint8_t c, uint8_t s) { /* include/fedagg_mx.h, "decode" */
  const int E = (c >> 3) & 15, m = c & 7;
  const float v = E ? ldexpf((float)(8 + m), E - 10) : ldexpf((float)m, -9);
  return ldexpf((c & 0x80) ? -v : v, (int)s - 127);
}

int main(int argc, char** argv) {
  const int device = argc > 1 ? atoi(argv[1]) : 0;
  const uint64_t nb = (M + FEDAGG_MX_BLOCK - 1) / FEDAGG_MX_BLOCK;
  const uint64_t ld_c = (M + 255) / 256 * 256, ld_s = (nb + 255) / 256 * 256;
  uint8_t* codes[K];
  uint8_t* scales[K];
  const void *seg_c[K], *seg_s[K];
  uint32_t seed = 777u;
  long long n[K], n_all = 0;
  for (int k = 0; k < K; ++k) {
    n[k] = 1 + (long long)(lcg(&seed) % 5000u);
    n_all += n[k];
    codes[k] = malloc(M);
    scales[k] = malloc(nb);
    for (uint64_t e = 0; e < M; ++e) {
      const uint32_t r = lcg(&seed) >> 8;
      codes[k][e] = (uint8_t)((1 + r % 0x7E) | ((r >> 16) & 0x80)); /* magnitudes 0x01 .. 0x7E: no zero, no NaN */
    }
    for (uint64_t b = 0; b < nb; ++b) scales[k][b] = (uint8_t)(100 + (lcg(&seed) >> 8) % 50);
    seg_c[k] = codes[k];
    seg_s[k] = scales[k];
  }
  float w[K];
  for (int k = 0; k < K; ++k) w[k] = (float)((double)n[k] / (double)n_all); /* fl32(n_k / n) */
  const uint64_t idx[2] = {31, M - 1};

  fedagg_session* s = fedagg_session_create(device);
  if (!s) {
    fprintf(stderr, "session_create: %s\n", fedagg_last_error());
    return 2;
  }
  void *d_codes = NULL, *d_scales = NULL, *d_out = NULL;
  const uint64_t bytes_c = M, bytes_s = nb;
  if (fedagg_session_buffer(s, 0, K * ld_c, &d_codes) || fedagg_session_buffer(s, 1, K * ld_s, &d_scales) ||
      fedagg_session_buffer(s, 2, ld_c * sizeof(float), &d_out) ||
      fedagg_session_stage(s, d_codes, ld_c, K, 1, seg_c, &bytes_c) ||
      fedagg_session_stage(s, d_scales, ld_s, K, 1, seg_s, &bytes_s)) {
    fprintf(stderr, "session: %s\n", fedagg_last_error());
    return 2;
  }
  const uint8_t *row_c[K], *row_s[K];
  for (int k = 0; k < K; ++k) {
    row_c[k] = (const uint8_t*)d_codes + k * ld_c;
    row_s[k] = (const uint8_t*)d_scales + k * ld_s;
  }
  int tile = 0, group = 0;
  fedagg_mx_blocking(&tile, &group);
  if (fedagg_mx_fedavg_e4m3(row_c, row_s, w, K, M, idx, 2, (float*)d_out, fedagg_session_stream(s))) {
    fprintf(stderr, "mx_fedavg_e4m3: %s\n", fedagg_mx_last_error());
    return 2;
  }
  float* got = malloc(M * sizeof(float));
  memset(got, 0xA5, M * sizeof(float));
  if (fedagg_session_fetch(s, d_out, got, M * sizeof(float))) {
    fprintf(stderr, "session_fetch: %s\n", fedagg_last_error());
    return 2;
  }
  /* a misaligned code row is refused before anything is launched */
  row_c[1] += 8;
  const int refused = fedagg_mx_fedavg_e4m3(row_c, row_s, w, K, M, idx, 2, (float*)d_out, fedagg_session_stream(s));
  fedagg_session_destroy(s);

  int bad = 0;
  for (uint64_t e = 0; e < M; ++e) {
    float acc = 0.0f;
    for (int k = 0; k < K; ++k) {
      const float x = decode(codes[k][e], scales[k][e / FEDAGG_MX_BLOCK]);
      const float p = x * w[k];
      acc = acc + p;
    }
    bad += memcmp(&acc, &got[e], sizeof(float)) != 0;
  }
  printf("fedavg_mx_demo: K=%d M=%u tile=%d k_group=%d mismatches=%d refused=%d (abi %d, mx abi %d)\n", K, M, tile, group,
         bad, refused, fedagg_abi_version(), fedagg_mx_abi_version());
  return (bad || refused != FEDAGG_EINVAL) ? 1 : 0;
}
