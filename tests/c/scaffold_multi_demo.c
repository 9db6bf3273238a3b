/* Scaffold on the one-call multi-device entry from plain C (no HIP headers, no Python): one
 * aggregation = fedagg_multi_scaffold_bucket twice (phase 0 the delta bucket, phase 1 the
 * control-variate bucket with K host copies of c, checked while they are staged), over {0, 0} and
 * over {0, 0, 0} (shards on one GPU, each with its own session), against the single-device path
 * (fedagg_session_stage of the same rows + fedagg_scaffold_f32 over the whole range), byte for byte.
 * Layers of ragged sizes with a (1,)-shaped one in the middle; a small "max_shard_bytes" makes every
 * shard stream through its GPU in several sub-ranges.  A second pass alters one element of one
 * client's c: the outputs stay those of copy 0 and the count is 1.
 * Usage: scaffold_multi_demo [dev]      (the device the shards run on, default 0)
 * Build: gcc -O2 -ffp-contract=off -Iinclude tests/c/scaffold_multi_demo.c -Lsubstrafl_amd -lfedagg */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fedagg.h"

#define K 10
#define NSEG 4
static const uint64_t numel[NSEG] = {7001, 1, 10000, 3003}; /* M = 20005; the (1,) layer at 7001 */

static uint32_t lcg(uint32_t* s) { return *s = *s * 1664525u + 1013904223u; }

static int fail(const char* what) {
  fprintf(stderr, "%s: %s\n", what, fedagg_last_error());
  return 2;
}

int main(int argc, char** argv) {
  const int dev = argc > 1 ? atoi(argv[1]) : 0;
  uint64_t M = 0, seg_bytes[NSEG];
  for (int i = 0; i < NSEG; ++i) {
    M += numel[i];
    seg_bytes[i] = numel[i] * sizeof(float);
  }
  /* per client: delta, control-variate update and its own copy of the server control variate */
  static float* delta[K][NSEG];
  static float* cv[K][NSEG];
  static float* c[K][NSEG];
  const void *seg_d[K * NSEG], *seg_cv[K * NSEG], *seg_c[K * NSEG];
  uint32_t seed = 4242u;
  long long n[K], n_all = 0;
  for (int k = 0; k < K; ++k) {
    n[k] = 1 + (long long)(lcg(&seed) % 5000u);
    n_all += n[k];
    for (int i = 0; i < NSEG; ++i) {
      delta[k][i] = malloc(seg_bytes[i]);
      cv[k][i] = malloc(seg_bytes[i]);
      c[k][i] = malloc(seg_bytes[i]);
      for (uint64_t e = 0; e < numel[i]; ++e) {
        delta[k][i][e] = ((float)(int32_t)lcg(&seed)) * 1e-9f;
        cv[k][i][e] = ((float)(int32_t)lcg(&seed)) * 1e-9f;
      }
      seg_d[k * NSEG + i] = delta[k][i];
      seg_cv[k * NSEG + i] = cv[k][i];
      seg_c[k * NSEG + i] = c[k][i];
    }
  }
  for (int i = 0; i < NSEG; ++i) {
    for (uint64_t e = 0; e < numel[i]; ++e) c[0][i][e] = ((float)(int32_t)lcg(&seed)) * 1e-9f;
    for (int k = 1; k < K; ++k) memcpy(c[k][i], c[0][i], seg_bytes[i]);
  }
  double w[K];
  for (int k = 0; k < K; ++k) w[k] = (double)n[k] / (double)n_all; /* scaffold.py:319-320 */
  const double lr = 0.7;
  uint64_t idx[1] = {numel[0]};

  /* the single-device call over the whole range */
  double* one_d = calloc(M, sizeof(double));
  double* one_c = calloc(M, sizeof(double));
  fedagg_session* s = fedagg_session_create(dev);
  if (!s) return fail("session");
  const uint64_t ld = (M + 63) / 64 * 64;
  void *d_d = NULL, *d_cv = NULL, *d_c = NULL, *d_od = NULL, *d_oc = NULL, *d_ws = NULL;
  if (fedagg_session_buffer(s, 0, K * ld * sizeof(float), &d_d) ||
      fedagg_session_buffer(s, 1, K * ld * sizeof(float), &d_cv) ||
      fedagg_session_buffer(s, 2, ld * sizeof(float), &d_c) ||
      fedagg_session_buffer(s, 3, ld * sizeof(double), &d_od) ||
      fedagg_session_buffer(s, 4, ld * sizeof(double), &d_oc) ||
      fedagg_session_buffer(s, 5, fedagg_pairwise_ws_bytes(K, 1, 8), &d_ws) ||
      fedagg_session_stage(s, d_d, ld * sizeof(float), K, NSEG, seg_d, seg_bytes) ||
      fedagg_session_stage(s, d_cv, ld * sizeof(float), K, NSEG, seg_cv, seg_bytes) ||
      fedagg_session_stage(s, d_c, ld * sizeof(float), 1, NSEG, seg_c, seg_bytes))
    return fail("stage");
  const float *rows_d[K], *rows_cv[K];
  for (int k = 0; k < K; ++k) {
    rows_d[k] = (const float*)((const char*)d_d + k * ld * sizeof(float));
    rows_cv[k] = (const float*)((const char*)d_cv + k * ld * sizeof(float));
  }
  if (fedagg_scaffold_f32(rows_d, rows_cv, (const float*)d_c, w, K, M, idx, 1, d_ws, lr, (double*)d_od,
                          (double*)d_oc, fedagg_session_stream(s)) ||
      fedagg_session_fetch(s, d_od, one_d, sizeof(double) * M) ||
      fedagg_session_fetch(s, d_oc, one_c, sizeof(double) * M))
    return fail("scaffold_f32");
  fedagg_session_destroy(s);

  /* the multi-device path: two shards, then three */
  int bad_d = 0, bad_c = 0, clean = 0, altered = 0, bad_altered = 0, ranges_total = 0, shards_used = 0;
  double* out_d = malloc(M * sizeof(double));
  double* out_c = malloc(M * sizeof(double));
  for (int ndev = 2; ndev <= 3; ++ndev) {
    int devs[3] = {dev, dev, dev};
    fedagg_multi* m = fedagg_multi_create(ndev, devs, 0);
    if (!m) return fail("multi_create");
    /* K x 4 + 8 (+ 4) B per element: 1024 elements per sub-range, several per shard */
    if (fedagg_multi_set(m, "max_shard_bytes", 64 << 10)) return fail("multi_set");
    memset(out_d, 0xA5, M * sizeof(double));
    memset(out_c, 0xA5, M * sizeof(double));
    uint64_t mism = 99;
    if (fedagg_multi_scaffold_bucket(m, 0, K, NSEG, seg_d, seg_bytes, FEDAGG_F32, w, lr, 0, 0, NULL, NULL, 0, idx, 1,
                                     out_d, NULL))
      return fail("multi_scaffold_bucket (delta)");
    for (int g = 0; g < ndev; ++g) {
      int ranges = 0;
      uint64_t lo = 0, hi = 0;
      if (fedagg_multi_shard_info(m, g, NULL, NULL, NULL, NULL, &lo, &hi, &ranges)) return fail("shard_info");
      printf("%d shards, shard %d: range [%llu, %llu) sub-ranges %d\n", ndev, g, (unsigned long long)lo,
             (unsigned long long)hi, ranges);
      ranges_total += ranges;
      shards_used += hi > lo;
    }
    if (fedagg_multi_scaffold_bucket(m, 1, K, NSEG, seg_cv, seg_bytes, FEDAGG_F32, w, lr, K, NSEG, seg_c, seg_bytes,
                                     FEDAGG_F32, idx, 1, out_c, &mism))
      return fail("multi_scaffold_bucket (control variate)");
    clean += (int)mism;
    for (uint64_t e = 0; e < M; ++e) {
      bad_d += memcmp(&out_d[e], &one_d[e], sizeof(double)) != 0;
      bad_c += memcmp(&out_c[e], &one_c[e], sizeof(double)) != 0;
    }
    /* one client's copy of c differs in one element: counted, and the outputs are still written */
    const float kept = c[K - 2][2][9999];
    c[K - 2][2][9999] = kept + 1.0f;
    memset(out_c, 0xA5, M * sizeof(double));
    mism = 99;
    if (fedagg_multi_scaffold_bucket(m, 1, K, NSEG, seg_cv, seg_bytes, FEDAGG_F32, w, lr, K, NSEG, seg_c, seg_bytes,
                                     FEDAGG_F32, idx, 1, out_c, &mism))
      return fail("multi_scaffold_bucket (altered c)");
    c[K - 2][2][9999] = kept;
    altered += (int)mism;
    for (uint64_t e = 0; e < M; ++e) bad_altered += memcmp(&out_c[e], &one_c[e], sizeof(double)) != 0;
    fedagg_multi_destroy(m);
  }
  printf("scaffold_multi_demo: K=%d M=%llu used=%d sub_ranges=%d delta=%d c=%d mismatches=%d altered=%d "
         "c_after_altered=%d (abi %d)\n",
         K, (unsigned long long)M, shards_used, ranges_total, bad_d, bad_c, clean, altered, bad_altered,
         fedagg_abi_version());
  return (bad_d || bad_c || clean || altered != 2 || bad_altered || shards_used != 5 || ranges_total <= 5) ? 1 : 0;
}
