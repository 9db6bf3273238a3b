/* bf16 FedAvg on the one-call multi-device entry from plain C (no HIP headers, no Python):
 * fedagg_multi_fedavg_bf16 over `devs` (default {0, 0}: two shards on one GPU, each with its own
 * session) against the reference order on the host (fed_avg.py:217-222 on the exact fp32 upcast of
 * the rows: acc = +0.0; acc = fl(acc + fl(x_k * w_k)), all in float), bit for bit.  Rows of bf16 bit
 * patterns in two uneven segments; a small "max_shard_bytes" makes every shard stream through its
 * GPU in several sub-ranges; two numel == 1 indices, one on a sub-range edge and one at a shard's
 * first element (K < 8, so NumPy's pairwise order over the K products is the plain one and the
 * host loop covers them too: no product here is a zero).
 * Usage: fedavg_multi_bf16_demo [dev0 dev1 ...]
 * Build: gcc -O2 -ffp-contract=off -Iinclude tests/c/fedavg_multi_bf16_demo.c -Lsubstrafl_amd -lfedagg */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fedagg.h"

#define K 5
#define NSEG 2
static const uint64_t numel[NSEG] = {7001, 13004}; /* M = 20005 */

static uint32_t lcg(uint32_t* s) { return *s = *s * 1664525u + 1013904223u; }

static float upcast(uint16_t b) { /* bf16 -> fp32, exact */
  uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, sizeof(f));
  return f;
}

int main(int argc, char** argv) {
  int devs[16] = {0, 0};
  int ndev = 2;
  if (argc > 1) {
    ndev = argc - 1 > 16 ? 16 : argc - 1;
    for (int g = 0; g < ndev; ++g) devs[g] = atoi(argv[g + 1]);
  }
  uint64_t M = 0, seg_bytes[NSEG];
  for (int i = 0; i < NSEG; ++i) {
    M += numel[i];
    seg_bytes[i] = numel[i] * sizeof(uint16_t);
  }
  uint16_t* layers[K][NSEG];
  const void* seg[K * NSEG];
  uint32_t seed = 4242u;
  long long n[K], n_all = 0;
  for (int k = 0; k < K; ++k) {
    n[k] = 1 + (long long)(lcg(&seed) % 5000u);
    n_all += n[k];
    for (int i = 0; i < NSEG; ++i) {
      layers[k][i] = malloc(seg_bytes[i]);
      for (uint64_t e = 0; e < numel[i]; ++e) {
        /* a value in (-2.2, 2.2), never zero, truncated to bf16: the upper half of its fp32 bits */
        const float f = ((float)(int32_t)(lcg(&seed) | 1u)) * 1e-9f;
        uint32_t u;
        memcpy(&u, &f, sizeof(u));
        layers[k][i][e] = (uint16_t)(u >> 16);
      }
      seg[k * NSEG + i] = layers[k][i];
    }
  }
  float w[K];
  for (int k = 0; k < K; ++k) w[k] = (float)((double)n[k] / (double)n_all); /* fl32(n_k / n) */
  const uint64_t idx[2] = {2047, 10240};

  fedagg_multi* m = fedagg_multi_create(ndev, devs, 0);
  if (!m) {
    fprintf(stderr, "multi_create: %s\n", fedagg_last_error());
    return 2;
  }
  float* multi = malloc(M * sizeof(float));
  float* again = malloc(M * sizeof(float));
  memset(multi, 0xA5, M * sizeof(float));
  memset(again, 0xA5, M * sizeof(float));
  /* K x 2 + 4 = 14 B per element: 2048 elements per sub-range, several per shard */
  if (fedagg_multi_set(m, "max_shard_bytes", 14 * 2048) ||
      fedagg_multi_fedavg_bf16(m, K, NSEG, seg, seg_bytes, w, idx, 2, multi)) {
    fprintf(stderr, "multi_fedavg_bf16: %s\n", fedagg_last_error());
    return 2;
  }
  int ranges_total = 0, shards_used = 0;
  for (int g = 0; g < ndev; ++g) {
    int dev = -1, node = -2, threads = 0, ncpus = 0, ranges = 0;
    uint64_t lo = 0, hi = 0;
    if (fedagg_multi_shard_info(m, g, &dev, &node, &threads, &ncpus, &lo, &hi, &ranges)) {
      fprintf(stderr, "shard_info: %s\n", fedagg_last_error());
      return 2;
    }
    printf("shard %d: device %d numa %d threads %d cpus %d range [%llu, %llu) sub-ranges %d\n", g, dev, node, threads,
           ncpus, (unsigned long long)lo, (unsigned long long)hi, ranges);
    ranges_total += ranges;
    shards_used += hi > lo;
  }
  /* a second call on the same object under the default budget (grow-only buffers reused): the same bits */
  if (fedagg_multi_set(m, "max_shard_bytes", 0) || fedagg_multi_fedavg_bf16(m, K, NSEG, seg, seg_bytes, w, idx, 2, again)) {
    fprintf(stderr, "multi_fedavg_bf16 (2): %s\n", fedagg_last_error());
    return 2;
  }
  fedagg_multi_destroy(m);

  int bad = 0, bad_again = 0;
  uint64_t base = 0;
  for (int i = 0; i < NSEG; ++i) {
    for (uint64_t e = 0; e < numel[i]; ++e) {
      float acc = 0.0f;
      for (int k = 0; k < K; ++k) {
        float p = upcast(layers[k][i][e]) * w[k];
        acc = acc + p;
      }
      bad += memcmp(&acc, &multi[base + e], sizeof(float)) != 0;
      bad_again += memcmp(&again[base + e], &multi[base + e], sizeof(float)) != 0;
    }
    base += numel[i];
  }
  printf("fedavg_multi_bf16_demo: K=%d M=%llu shards=%d sub_ranges=%d mismatches=%d again=%d used=%d (abi %d)\n", K,
         (unsigned long long)M, ndev, ranges_total, bad, bad_again, shards_used, fedagg_abi_version());
  return (bad || bad_again || ranges_total <= ndev) ? 1 : 0;
}
