/*
 * fedagg_mx.h -- C ABI of libfedagg_mx.so: FedAvg over OCP MXFP8 client updates, and the
 * quantiser that produces them, on MI355X (gfx950).
 *
 * A client update on the MXFP8 wire is 1-byte e4m3fn elements ("codes") with one e8m0
 * power-of-two scale byte per block of 32 consecutive elements of the flat bucket: 1.03 bytes per
 * parameter on the wire, over PCIe and in HBM, against 4 for fp32 and 2 for bf16.  Decoding is
 * exact in fp32, so the aggregation keeps the contract of fedagg_fedavg_bf16: bit-identical to the
 * reference's FedAvg arithmetic (fed_avg.py:217-222) run on the exactly decoded fp32 inputs.
 *
 * A library of its own beside libfedagg.so: nothing in fedagg.h changes, and only an MXFP8 call
 * loads it.  The kinds (FEDAGG_F32, FEDAGG_BF16) and the return codes are those of fedagg.h.
 *
 * The format
 *   decode  A code c has sign S, exponent field E (4 bits), mantissa field m (3 bits):
 *             v = (-1)^S * m * 2^-9            if E == 0
 *             v = (-1)^S * (8 + m) * 2^(E-10)  otherwise
 *           0x7F and 0xFF are NaN; there is no infinity (e4m3fn, not fnuz).  With the scale byte s
 *           of the element's block, x = fl32(v * 2^(s-127)); s == 255 makes the whole block NaN.
 *           Every finite product is an fp32 value, down to the subnormals (the smallest granule is
 *           2^-136); nothing is flushed.  The one inexact case is overflow to +-inf (448 * 2^127).
 *   encode  Per block, amax = max |x_i|:
 *             any NaN or Inf in the block:  s = 255, every code 0x00
 *             amax == 0:                    s = 127, the codes carry the zeros' signs
 *             otherwise:  e = floor(log2(amax)) - 8;  e += 1 if amax * 2^-e > 464 (the tie that
 *                         still rounds to 448: nothing saturates);  e clamped to [-127, 127];
 *                         s = e + 127
 *           An element is y = fl32(x * 2^-e) rounded to nearest even among the e4m3fn values,
 *           |y| >= 448 to +-448, the sign of zero kept.
 *   blocks  Block b covers flat elements [32 b, min(32 b + 32, M)) of a row.
 * substrafl_amd/wire.py restates both rules in NumPy; the tests hold the kernels to it bit for bit
 * (NaN by position: payloads are unspecified).
 *
 * Conventions (those of fedagg.h and fedagg_promote.h)
 *   - d_* are device pointers owned by the caller; the pointer tables, h_w and h_idx are host
 *     arrays, read before the call returns.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream); every call is asynchronous on
 *     it, allocates nothing and never synchronises the host, so it may be captured into a graph.
 *   - Every argument is checked before the first HIP call: a refused call has launched nothing.
 *     Return: 0, or a negative code with fedagg_mx_last_error() giving the calling thread's
 *     message.  M == 0 returns FEDAGG_OK and touches nothing.
 */
#ifndef FEDAGG_MX_H
#define FEDAGG_MX_H

#include <stddef.h>
#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FEDAGG_MX_ABI_VERSION 1
#define FEDAGG_MX_BLOCK 32            /* elements per scale byte                                   */
#define FEDAGG_MX_KCHUNK 128          /* clients per launch (kernel-argument table)                */
#define FEDAGG_MX_MAX_PAIRWISE_K 256  /* clients up to which numel == 1 elements are served        */

int fedagg_mx_abi_version(void);
const char* fedagg_mx_last_error(void);

/* The sizes at which the FedAvg kernel changes path: a workgroup step covers *tile_elems
 * consecutive elements (whole tiles take the unrolled walk, the last partial tile goes vector by
 * vector and the last M % 16 elements one by one), and clients are loaded *k_group at a time ahead
 * of the in-order add chain (the last K % k_group clients one by one).  Either pointer may be NULL. */
int fedagg_mx_blocking(int* tile_elems, int* k_group);

/* FedAvg over K MXFP8 rows of M elements: d_codes[k] the M code bytes of client k, d_scales[k] its
 * ceil(M / 32) scale bytes.  For every element: decode as above, then fedagg_fedavg_f32's
 * arithmetic exactly,
 *     acc = +0.0;  for k in 0..K-1 (list order):  acc = fl32(acc + fl32(x_k[i] * h_w[k]))
 * with h_w[k] = fl32(n_k / n); the decode and the weight product are two roundings, never merged.
 * The P flat indices in h_idx (numel == 1 layers; may be NULL when P == 0) take
 *     out = +0.0 + pairwise_sum(p_0 .. p_{K-1})
 * with NumPy's pairwise tree instead, in a second small kernel.  There is no workspace argument:
 * the tree's two halves of K <= FEDAGG_MX_MAX_PAIRWISE_K clients need none, and P > 0 with more
 * clients is FEDAGG_EINVAL.  More than FEDAGG_MX_KCHUNK clients continue the accumulator in d_out.
 * Code rows must be 16-B aligned (FEDAGG_EINVAL otherwise); scale rows and M are arbitrary; d_out
 * is 4-B aligned (16-B aligned for the vector path, else every element goes one by one).
 * FEDAGG_EINVAL, each with its own text: K <= 0, NULL d_codes / d_scales / h_w / d_out, a NULL or
 * misaligned row, P < 0, NULL h_idx with P > 0, an index >= M, P > 0 with K above the limit. */
int fedagg_mx_fedavg_e4m3(const uint8_t* const* d_codes, const uint8_t* const* d_scales, const float* h_w, int K,
                          uint64_t M, const uint64_t* h_idx, int P, float* d_out, void* stream);

/* Encode M elements of d_x (kind FEDAGG_F32, or FEDAGG_BF16 widened exactly first; any other kind
 * is FEDAGG_EINVAL) by the rule above: M code bytes to d_codes, ceil(M / 32) scale bytes to
 * d_scales.  No atomics: the 32 lanes of a block exchange the block maximum.  d_x needs its
 * element's alignment only; d_codes and d_scales are arbitrary. */
int fedagg_mx_quantize(const void* d_x, int kind, uint64_t M, uint8_t* d_codes, uint8_t* d_scales, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDAGG_MX_H */
