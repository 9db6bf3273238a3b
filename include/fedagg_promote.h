/*
 * fedagg_promote.h -- C ABI of libfedagg_promote.so: the client flat ops of a 16-bit model next to
 * fp64 operands, on MI355X (gfx950).
 *
 * From round 2 on a Scaffold client of a model.half() / model.to(torch.bfloat16) model works on
 * fp64 lists (the aggregator's avg_parameters_update and server_control_variate) next to its own
 * 16-bit ones, and torch's type promotion defines every such op of the reference's
 * weight_manager.py (:103-137 increment_parameters, :182-212 weighted_sum_parameters).  These two
 * entry points are those ops over a flat fp64 bucket: one launch per 32 layers instead of two
 * torch launches per layer.
 *
 * A library of its own beside libfedagg.so: nothing in fedagg.h changes (fedagg_flat_wsum and
 * fedagg_flat_increment_kind keep refusing these operand sets), and only a 16-bit model that
 * meets an fp64 operand loads it.  The kinds (FEDAGG_F16, FEDAGG_BF16, FEDAGG_F32, FEDAGG_F64),
 * FEDAGG_FLAT_MAX_LISTS and the return codes are those of fedagg.h.
 *
 * Arithmetic: torch's, bit for bit (T is the one 16-bit kind of the call, fl_T / fl32 round to
 * nearest even, overflow to +-inf; NaN stays NaN, payloads unspecified; nothing is flushed;
 * every product and sum is rounded on its own, never contracted).
 *   wsum: Python sum() from int 0 over x_j * c_j, list by list in the order given
 *     product of a 16-bit list:  p_j = fl_T(fl32(x_j) * fl32(c_j))   (the Python scalar rounded to
 *                                fp32, the product rounded once to T)
 *     product of an fp64 list:   p_j = x_j * c_j in fp64, c_j the double it is
 *     first term:                acc = 0 + p_0 in p_0's own kind; 16-bit: fl_T(0.0f + fl32(p_0)),
 *                                so -0 becomes +0 (in fp64 as well)
 *     later term, both 16-bit:   acc = fl_T(fl32(acc) + fl32(p_j))
 *     later term, either fp64:   the 16-bit side widened exactly, the sum in fp64; acc is fp64
 *                                from there on.  The result (d_flat) is fp64.
 *   increment: t = multiplier * u in fp64, then w = fl_T(fl32(fl64(w) + t)).  torch converts a
 *     double to Half / BFloat16 THROUGH float: two roundings, and they stay two here
 *     (w = 1, t = 2^-11 + 2^-40 gives fp16 0x3C00, where one rounding would give 0x3C01).
 * The yardstick is torch on the device, on per-layer tensors of their own as the reference
 * creates them (tests/test_promote_ops_gpu.py); tests/promote_rules.py restates the rules in
 * single-dtype ops and is held to torch on the CPU over all 65536 bit patterns of each kind.
 * Torch on the device (ROCm, torch 2.10, MI355X) leaves these rules on ONE class of elements, and
 * the kernels follow it there:
 *   fp16 product, remainder of a layer: torch serves a contiguous 16-B aligned fp16 tensor in
 *     blocks of 2048 elements; the tensor's last numel mod 2048 elements (a whole tensor below 2048)
 *     go through an unrolled loop whose multiply and conversion are one fused operation.  There
 *     p_j = fl_f16(x_j * fl32(c_j)) with the EXACT product rounded once (not fl32 first), and an
 *     exact zero product is +0 whatever the signs.  So for layer l of an F16 list, elements
 *     [floor(numel[l] / 2048) * 2048, numel[l]) take that form and the elements before them the
 *     rule above.  The two differ only where the fp32 product lands on an fp16 rounding tie (c
 *     such as 0.3 or 1 / 0.15, never a power of two), about 1 element in 10^4 there.
 *   Measured equal to the rules everywhere else: bf16 products, every sum, every fp64 step, and
 *   the whole of the increment (a mixed double operand takes torch's generic loop, which has no
 *   vectorised specialisation), over the values and geometries of the GPU test.
 *
 * Conventions (those of fedagg.h)
 *   - d_* are device pointers owned by the caller; numel / kinds / coeffs and the pointer array
 *     itself are host memory, read before the call returns.
 *   - d_layers is list-major [nlists][L]; layer l of every list has numel[l] elements; the layers'
 *     results lie back to back in d_flat (layer l at element numel[0] + ... + numel[l-1]).
 *   - `stream` is a hipStream_t (NULL = the legacy default stream); every call is asynchronous on
 *     it, allocates nothing and never synchronises the host, so it may be captured into a graph.
 *   - Every argument is checked before the first HIP call: a refused call has launched nothing.
 *     Return: 0, or a negative code with fedagg_promote_last_error() giving the calling thread's
 *     message.  L == 0 (or every numel 0) returns FEDAGG_OK and touches nothing.
 *   - 16-bit pointers must be 2-B aligned, fp64 pointers and d_flat 8-B aligned.  A layer whose
 *     16-bit pointers are all 16-B aligned moves 8 elements per lane (16 B of each 16-bit operand,
 *     4 x 16 B of each fp64 operand, declared 8-B aligned: a layer's slice of the bucket starts
 *     wherever the previous layers end); every other layer, and the last < 8 elements of each
 *     8192-element chunk, go element by element.  Both forms give the same bits.
 */
#ifndef FEDAGG_PROMOTE_H
#define FEDAGG_PROMOTE_H

#include <stddef.h>
#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FEDAGG_PROMOTE_ABI_VERSION 1

int fedagg_promote_abi_version(void);
const char* fedagg_promote_last_error(void);

/* Knobs, for the tests: "vec" 1 (default) / 0 = every layer element by element.  Process-wide;
 * an unknown key or value is FEDAGG_EINVAL. */
int fedagg_promote_tune(const char* key, int value);

/* d_flat (fp64) = sum() of list_j * coeffs[j].  kinds[j] is the kind of list j: every list is
 * FEDAGG_F64 or the call's one 16-bit kind, with at least one list of each sort.  FEDAGG_EINVAL,
 * each with its own text: an fp32 list (fedagg_flat_wsum serves fp32 next to fp64), F16 next to
 * BF16, any other kind, no 16-bit list, no fp64 list, nlists outside 1..FEDAGG_FLAT_MAX_LISTS,
 * L < 0, a NULL array or a NULL layer with numel > 0, a misaligned pointer.  coeffs NULL: all 1. */
int fedagg_promote_wsum(const void* const* d_layers, const int* kinds, int nlists, const double* coeffs,
                        const uint64_t* numel, int L, double* d_flat, void* stream);

/* w += multiplier * u: the layers (layer_kind FEDAGG_F16 or FEDAGG_BF16, any other kind is
 * FEDAGG_EINVAL: fedagg_flat_increment keeps fp32 parameters) updated in place from the fp64
 * bucket d_flat, which is only read. */
int fedagg_promote_increment(void* const* d_layers, int layer_kind, const uint64_t* numel, int L,
                             const double* d_flat, double multiplier, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDAGG_PROMOTE_H */
