/*
 * fedagg_mx4.h -- C ABI of libfedagg_mx4.so: FedAvg over OCP MXFP4 client updates, and the
 * quantiser that produces them (with or without error feedback), on MI355X (gfx950).
 *
 * A client update on the MXFP4 wire is 4-bit e2m1 elements ("codes"), two to a byte, with one e8m0
 * power-of-two scale byte per block of 32 consecutive elements of the flat bucket: 0.53 bytes per
 * parameter on the wire, over PCIe and in HBM, against 1.03 for MXFP8 (fedagg_mx.h), 2 for bf16 and
 * 4 for fp32.  Decoding is exact in fp32, so the aggregation keeps the contract of
 * fedagg_mx_fedavg_e4m3: bit-identical to the reference's FedAvg arithmetic run on the exactly
 * decoded fp32 inputs.  A 4-bit element keeps one mantissa bit; the error feedback of
 * fedagg_mxef.h, here an argument of the one quantiser, is what makes such an update usable.
 *
 * A library of its own beside libfedagg.so, libfedagg_mx.so and libfedagg_mxef.so: nothing in
 * their headers changes, and only an MXFP4 call loads it.  The kinds (FEDAGG_F32, FEDAGG_BF16) and
 * the return codes are those of fedagg.h.
 *
 * The format
 *   element e2m1: 1 sign bit (bit 3), 2 exponent bits, 1 mantissa bit.  The magnitudes of the codes
 *           0..7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6.  There is no NaN and no infinity.
 *   packing Two codes share a byte: flat element 2 j is in bits 3:0 of byte j, element 2 j + 1 in
 *           bits 7:4.  A row of M elements is ceil(M / 2) bytes; the unused high nibble of an odd M
 *           is written as 0 and never read.
 *   blocks  Block b covers flat elements [32 b, min(32 b + 32, M)) of a row: 16 bytes of codes and
 *           one scale byte s, over the raveled concatenation of the layers with no padding.
 *   decode  x = fl32(v * 2^(s-127)); s == 255 makes the whole block NaN.  Every finite product is an
 *           fp32 value, down to the subnormals (the smallest granule is 2^-128); nothing is
 *           flushed.  The one inexact case is overflow to +-inf: |v| >= 2 under s = 254, which the
 *           encoder never produces, and |v| >= 4 under s = 253, which it produces for a block
 *           maximum of 3.5 * 2^126 and above.
 *   encode  Per block, amax = max |x_i|:
 *             any NaN or Inf in the block:  s = 255, every code 0
 *             amax == 0:                    s = 127, the codes carry the zeros' signs
 *             otherwise:  e = floor(log2(amax)) - 2;  e += 1 if amax * 2^-e >= 7 (the tie that
 *                         rounds to the missing 8: after the bump nothing saturates);  e clamped to
 *                         [-127, 127];  s = e + 127
 *           An element is y = fl32(x * 2^-e) rounded to nearest even among the e2m1 values (the ties
 *           0.25, 0.75, 1.25, 1.75, 2.5, 3.5 and 5 go to the even codes 0, 2, 2, 4, 4, 6, 6),
 *           |y| >= 6 to +-6, the sign of zero kept.
 *   error feedback  The rule of fedagg_mxef.h: r = fl32(x + res), (codes, scales) = encode(r),
 *           d = decode, res' = fl32(r - d) where the block is finite (s != 255) and d is finite,
 *           res' = +0.0 otherwise: a non-finite block's residual is dropped, so it cannot poison
 *           every later round.  The residual is fp32 for bf16 updates too.  Wherever d is finite,
 *           r - d is exact in fp32.
 * substrafl_amd/wire.py restates these rules in NumPy; the tests hold the kernels to it bit for bit
 * (NaN by position: payloads are unspecified).
 *
 * Conventions (those of fedagg_mx.h)
 *   - d_* are device pointers owned by the caller; the pointer tables, h_w and h_idx are host
 *     arrays, read before the call returns.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream); every call is asynchronous on
 *     it, allocates nothing and never synchronises the host, so it may be captured into a graph.
 *   - Every argument is checked before the first HIP call: a refused call has launched nothing.
 *     Return: 0, or a negative code with fedagg_mx4_last_error() giving the calling thread's
 *     message.  M == 0 returns FEDAGG_OK and touches nothing.
 */
#ifndef FEDAGG_MX4_H
#define FEDAGG_MX4_H

#include <stddef.h>
#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FEDAGG_MX4_ABI_VERSION 1
#define FEDAGG_MX4_BLOCK 32            /* elements per scale byte                                  */
#define FEDAGG_MX4_KCHUNK 128          /* clients per launch (kernel-argument table)               */
#define FEDAGG_MX4_MAX_PAIRWISE_K 256  /* clients up to which numel == 1 elements are served       */

int fedagg_mx4_abi_version(void);
const char* fedagg_mx4_last_error(void);

/* The sizes at which the FedAvg kernel changes path: a workgroup step covers *tile_elems
 * consecutive elements (a lane one 32-element block; whole waves store through LDS, a partial wave
 * directly, and the last M % 32 elements go one by one), and clients are loaded *k_group at a time
 * ahead of the in-order add chain (the last K % k_group clients one by one).  Either pointer may be
 * NULL. */
int fedagg_mx4_blocking(int* tile_elems, int* k_group);

/* FedAvg over K MXFP4 rows of M elements: d_codes[k] the ceil(M / 2) code bytes of client k,
 * d_scales[k] its ceil(M / 32) scale bytes.  For every element: decode as above, then
 * fedagg_fedavg_f32's arithmetic exactly,
 *     acc = +0.0;  for k in 0..K-1 (list order):  acc = fl32(acc + fl32(x_k[i] * h_w[k]))
 * with h_w[k] = fl32(n_k / n); the decode and the weight product are two roundings, never merged.
 * The P flat indices in h_idx (numel == 1 layers; may be NULL when P == 0) take
 *     out = +0.0 + pairwise_sum(p_0 .. p_{K-1})
 * with NumPy's pairwise tree instead, in a second small kernel, up to FEDAGG_MX4_MAX_PAIRWISE_K
 * clients (P > 0 with more is FEDAGG_EINVAL).  More than FEDAGG_MX4_KCHUNK clients continue the
 * accumulator in d_out.  Code rows must be 16-B aligned (FEDAGG_EINVAL otherwise); scale rows and
 * M are arbitrary; d_out (M fp32) is 4-B aligned (16-B aligned for the vector path, else every
 * element goes one by one through the plain decoder).
 * FEDAGG_EINVAL, each with its own text: K <= 0, NULL d_codes / d_scales / h_w / d_out, a NULL or
 * misaligned row, P < 0, NULL h_idx with P > 0, an index >= M, P > 0 with K above the limit. */
int fedagg_mx4_fedavg_e2m1(const uint8_t* const* d_codes, const uint8_t* const* d_scales, const float* h_w, int K,
                           uint64_t M, const uint64_t* h_idx, int P, float* d_out, void* stream);

/* Encode M elements of d_x (kind FEDAGG_F32, or FEDAGG_BF16 widened exactly first; any other kind
 * is FEDAGG_EINVAL) by the rule above: ceil(M / 2) code bytes to d_codes, ceil(M / 32) scale bytes
 * to d_scales.  d_res NULL: the plain quantiser.  Otherwise d_res holds the M fp32 residuals: one
 * fused pass reads d_x and d_res once and writes the codes, the scales and the new residual over
 * d_res (in place) once, by the error-feedback rule above; d_res must not overlap d_x, d_codes or
 * d_scales.  No atomics.  d_x and d_res need their element's alignment only and d_codes, d_scales
 * any: the whole scale blocks of a call with d_x (and d_res) 16-B aligned and d_codes 4-B aligned
 * take the vector walk (8 elements per lane), everything else one element per lane, with identical
 * bits.
 * FEDAGG_EINVAL, each with its own text: a bad kind, M above 2^44, NULL d_x / d_codes / d_scales,
 * d_x or d_res not aligned to its element, d_res overlapping d_x, d_codes or d_scales. */
int fedagg_mx4_quantize(const void* d_x, int kind, uint64_t M, float* d_res, uint8_t* d_codes, uint8_t* d_scales,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDAGG_MX4_H */
