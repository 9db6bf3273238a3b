/*
 * fedagg_mxdl.h -- C ABI of libfedagg_mxdl.so: the MXFP8 downlink on MI355X (gfx950).
 *
 * The uplink of an MX federation carries 1.03 (MXFP8) or 0.53 (MXFP4) bytes per parameter
 * (fedagg_mx.h, fedagg_mx4.h).  This library closes the loop: the aggregator emits the average
 * already quantised to MXFP8, and a client applies such an average to its model without an fp32
 * bucket in between.
 *
 *   fedagg_mxdl_fedavg      average K MX rows and encode the average, one pass: K*1.03 + 1.03 bytes
 *                           of HBM traffic per parameter, where the fedavg entry of fedagg_mx.h
 *                           followed by fedagg_mx_quantize moves K*1.03 + 9.03
 *   fedagg_mxdl_increment   w += m * decode(codes, scales) over a model's fp32 parameter tensors:
 *                           9.03 bytes per parameter, against 17.03 for a decode into an fp32
 *                           bucket followed by fedagg_flat_increment
 *   fedagg_mxdl_decode      codes and scales to an fp32 row (for a bf16 model, whose increment
 *                           stays fedagg_flat_increment_kind)
 *
 * A library of its own beside libfedagg.so, libfedagg_mx.so, libfedagg_mxef.so and
 * libfedagg_mx4.so: nothing in their headers changes, and only a downlink call loads it.  The
 * return codes are those of fedagg.h; the format, the decode and the encode rule are those of
 * fedagg_mx.h (MXFP8) and fedagg_mx4.h (the MXFP4 input rows), unchanged.  The downlink carries no
 * residual: each call's output has the encoder's error of at most 2^-4 relative per element.
 *
 * Conventions (those of fedagg_mx.h)
 *   - d_* are device pointers owned by the caller; the pointer tables, h_w, h_idx and numel are
 *     host arrays, read before the call returns.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream); every call is asynchronous on
 *     it, allocates no device memory and never synchronises the host, so it may be captured into a
 *     graph.
 *   - Every argument is checked before the first HIP call: a refused call has launched nothing.
 *     Return: 0, or a negative code with fedagg_mxdl_last_error() giving the calling thread's
 *     message.  M == 0 returns FEDAGG_OK and touches nothing.
 */
#ifndef FEDAGG_MXDL_H
#define FEDAGG_MXDL_H

#include <stddef.h>
#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FEDAGG_MXDL_ABI_VERSION 1
#define FEDAGG_MXDL_E4M3 0    /* input rows: MXFP8, one e4m3fn code per byte (fedagg_mx.h)          */
#define FEDAGG_MXDL_E2M1 1    /* input rows: MXFP4, two e2m1 codes per byte (fedagg_mx4.h)          */
#define FEDAGG_MXDL_KMAX 128  /* clients per call: FEDAGG_MX_KCHUNK, the kernel-argument table      */

int fedagg_mxdl_abi_version(void);
const char* fedagg_mxdl_last_error(void);

/* The sizes at which the kernels change path: a lane owns *lane_elems consecutive elements (half
 * a scale block; whole ones take the vector walk, a partial last one goes element by element), a
 * workgroup step covers *tile_elems, and the fedavg kernel loads clients *k_group at a time ahead
 * of the in-order add chain (the last K % k_group clients one by one).  Any pointer may be NULL. */
int fedagg_mxdl_blocking(int* tile_elems, int* lane_elems, int* k_group);

/* FedAvg over K MX rows of M elements, the average encoded to MXFP8: M code bytes to d_out_codes,
 * ceil(M / 32) scale bytes to d_out_scales.  in_kind FEDAGG_MXDL_E4M3: d_codes[k] are the M code
 * bytes of client k as fedagg_mx_fedavg_e4m3 takes them; FEDAGG_MXDL_E2M1: its ceil(M / 2) packed
 * bytes as fedagg_mx4_fedavg_e2m1 takes them.  d_scales[k] are its ceil(M / 32) scale bytes.
 *
 * The output is fedagg_mx_quantize applied to avg, where avg is bit for bit the fp32 row that
 * fedagg_mx_fedavg_e4m3 (fedagg_mx4_fedavg_e2m1) gives for the same inputs:
 *     acc = +0.0;  for k in 0..K-1 (list order):  acc = fl32(acc + fl32(x_k[i] * h_w[k]))
 * the decode, the weight product and the add three roundings, never merged; the P flat indices in
 * h_idx (numel == 1 layers; may be NULL when P == 0) take +0.0 + pairwise_sum(p_0 .. p_{K-1}) with
 * NumPy's pairwise tree before the block they sit in is scaled (a second small kernel rewrites
 * those blocks).  avg itself never reaches memory.
 *
 * K is at most FEDAGG_MXDL_KMAX: a continued accumulator needs the fp32 row this entry removes (the
 * two entries named above serve more clients).  Input code rows must be 16-B aligned; the scale
 * rows, M and both output pointers are arbitrary (a d_out_codes that is not 16-B aligned is
 * written byte by byte, a d_out_scales that is not by one store per block: identical bits).
 * FEDAGG_EINVAL, each with its own text: an unknown in_kind, K <= 0, K > FEDAGG_MXDL_KMAX, NULL
 * d_codes / d_scales / h_w / d_out_codes / d_out_scales, a NULL or misaligned row, P < 0, NULL
 * h_idx with P > 0, an index >= M, M too large. */
int fedagg_mxdl_fedavg(int in_kind, const uint8_t* const* d_codes, const uint8_t* const* d_scales, const float* h_w,
                       int K, uint64_t M, const uint64_t* h_idx, int P, uint8_t* d_out_codes, uint8_t* d_out_scales,
                       void* stream);

/* w += m * decode(d_codes, d_scales) over the L fp32 tensors d_layers[l] of numel[l] elements, as
 * fedagg_flat_increment takes them; the M = sum of numel[l] codes run over the concatenation of
 * the raveled tensors, so a scale block may span two of them.  Per element
 *     w = fl32(w + fl32(fl32(multiplier) * d))
 * with d the exact decode, never contracted: the bits fedagg_flat_increment gives on the decoded
 * fp32 bucket.  Elements that lie 16 to a lane inside one tensor (with d_codes 16-B aligned) take
 * the vector walk, which starts at the lane's first 16-B aligned address of w wherever the tensor
 * begins; all others go one by one: identical bits.
 * FEDAGG_EINVAL, each with its own text: L < 0, NULL d_layers / numel with L > 0, a NULL tensor
 * with elements, a tensor that is not 4-B aligned or too large, numel that do not sum to M, NULL
 * d_codes / d_scales, M too large. */
int fedagg_mxdl_increment(float* const* d_layers, const uint64_t* numel, int L, const uint8_t* d_codes,
                          const uint8_t* d_scales, uint64_t M, double multiplier, void* stream);

/* The exact fp32 values of M codes under their ceil(M / 32) scale bytes, to d_out (4-B aligned;
 * 16-B aligned, with d_codes, for the vector walk).  FEDAGG_EINVAL, each with its own text: NULL
 * d_codes / d_scales / d_out, a misaligned d_out, M too large. */
int fedagg_mxdl_decode(const uint8_t* d_codes, const uint8_t* d_scales, uint64_t M, float* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDAGG_MXDL_H */
