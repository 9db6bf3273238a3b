/*
 * fedagg_mxef.h -- C ABI of libfedagg_mxef.so: the MXFP8 quantiser with error feedback, one fused
 * kernel on MI355X (gfx950).
 *
 * The MXFP8 wire of fedagg_mx.h is lossy: an element's error is up to about 6 % of its block's
 * maximum, and an element more than about five binades below that maximum rounds to zero every
 * round.  With error feedback the client keeps what the quantiser dropped (the residual, fp32, one
 * value per parameter) and adds it to the next round's update before quantising.  The wire format
 * and the aggregator do not change.
 *
 * A library of its own beside libfedagg_mx.so: nothing in fedagg_mx.h changes, and only a client
 * that asks for error feedback loads it.  The kinds (FEDAGG_F32, FEDAGG_BF16) and the return codes
 * are those of fedagg.h; the encode and decode rules and the blocks are those of fedagg_mx.h.
 *
 * The arithmetic (all fp32, no contraction), per element i of a flat bucket of M elements, block b
 * covering [32 b, min(32 b + 32, M)):
 *   r_i    = fl32(x_i + res_i)         x_i the fp32 element, or the bf16 element widened exactly
 *   (codes, scales) = the encode rule of fedagg_mx.h applied to r: the NaN/Inf-block rule
 *                     (s = 255, codes 0x00), the all-zero-block rule and the 464 bump unchanged
 *   d_i    = the decode of (code_i, s_b)
 *   res'_i = fl32(r_i - d_i)           when the block is finite (s_b != 255) and d_i is finite
 *   res'_i = +0.0                      otherwise: a non-finite block's residual is dropped, so it
 *                                      cannot poison every later round; and d_i can overflow to
 *                                      +-inf from finite input (|r| above 248 * 2^120 in a block
 *                                      bumped to e = 120 encodes to 256 and decodes to 2^128)
 * Facts of this rule, checked with substrafl_amd/wire.py:
 *   - Wherever d_i is finite, r_i - d_i is exact in fp32, subnormals included, so r_i = d_i + res'_i
 *     holds exactly: the only rounding error feedback adds is the one in x + res.
 *   - Over T rounds from res = 0 it follows in exact arithmetic, element by element, that
 *     |sum_t d_t + res_T - sum_t x_t| <= sum_t 2^-24 |r_t|.
 *   - With the same x sent 64 times the worst ratio of that gap to that bound was 0.56.
 *
 * Conventions (those of fedagg_mx.h)
 *   - d_* are device pointers owned by the caller.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream); the call is asynchronous on it,
 *     allocates nothing and never synchronises the host, so it may be captured into a graph.
 *   - Every argument is checked before the first HIP call: a refused call has launched nothing.
 *     Return: 0, or a negative code with fedagg_mxef_last_error() giving the calling thread's
 *     message.  M == 0 returns FEDAGG_OK and touches nothing.
 */
#ifndef FEDAGG_MXEF_H
#define FEDAGG_MXEF_H

#include <stddef.h>
#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FEDAGG_MXEF_ABI_VERSION 1

int fedagg_mxef_abi_version(void);
const char* fedagg_mxef_last_error(void);

/* The sizes at which the kernel changes path.  A lane of the vector walk owns *lane_elems
 * consecutive elements (a quarter of a scale block) and a workgroup step covers *tile_elems
 * consecutive elements.  The grid is capped, so with M above *second_step_elems some workgroup
 * takes a second step of its loop.  With one element per lane (see fedagg_mxef_quantize) a step
 * covers tile_elems / lane_elems elements and the second step begins at second_step_elems /
 * lane_elems.  Any pointer may be NULL. */
int fedagg_mxef_blocking(int* lane_elems, int* tile_elems, uint64_t* second_step_elems);

/* One fused pass over M elements: read d_x (kind FEDAGG_F32 or FEDAGG_BF16; any other kind is
 * FEDAGG_EINVAL) and the fp32 residual d_res once, write M code bytes to d_codes, ceil(M / 32)
 * scale bytes to d_scales and the new residual over d_res (in place) once, by the arithmetic above.
 * d_x and d_res need their element's alignment only and d_codes, d_scales any: the whole scale
 * blocks of a call with d_x and d_res 16-B aligned and d_codes 8-B aligned take the vector walk
 * (8 elements per lane), everything else one element per lane, with identical bits; a wave's 16
 * scale bytes leave as one 16-B store where d_scales is 16-B aligned.
 * d_res must not overlap d_x, d_codes or d_scales.
 * FEDAGG_EINVAL, each with its own text: a bad kind, M above 2^44, NULL d_x / d_res / d_codes /
 * d_scales, d_x or d_res not aligned to its element, d_res overlapping d_x, d_codes or d_scales. */
int fedagg_mxef_quantize(const void* d_x, int kind, uint64_t M, float* d_res, uint8_t* d_codes, uint8_t* d_scales,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDAGG_MXEF_H */
