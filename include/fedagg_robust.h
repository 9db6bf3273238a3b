/*
 * fedagg_robust.h -- C ABI of libfedagg_robust.so: the coordinate-wise trimmed mean over K client
 * rows, and the median as its limit case (Yin et al. 2018), on MI355X (gfx950).
 *
 * Every other aggregation of the engine is a weighted sum, so one client that sends a NaN, an Inf or
 * a diverged update reaches every parameter of the round.  Here each element drops its t lowest and
 * its t highest client values and averages the rest: up to t bad clients per element change nothing
 * but which values are kept.
 *
 * A library of its own beside libfedagg.so and the wire libraries: nothing in their headers changes,
 * and only a robust call loads it.  The kinds (FEDAGG_F32, FEDAGG_BF16) and the return codes are
 * those of fedagg.h.
 *
 * The rule, for every element i over the K client values x_0[i] .. x_{K-1}[i]
 *   order   ascending by value; -0.0 and +0.0 are equal; every NaN, of either sign and any payload,
 *           orders above +inf.  This is np.sort's order.
 *   window  the t lowest and the t highest are dropped, 0 <= 2 t < K.
 *   result  acc = +0.0;  for the kept values in ascending order:  acc = fl32(acc + v);
 *           out = fl32(acc / fl32(K - 2 t)), a correctly rounded fp32 division.  Nothing is
 *           contracted.  Starting from +0.0 makes the order among zeros irrelevant to the bits.
 *   NaN     up to t NaNs of an element are trimmed like any other extreme; more than t give NaN at
 *           that element (payload unspecified).
 *   t = 0 is the unweighted mean in sorted order; t = (K - 1) / 2 (integer division) the median:
 *   the middle value for odd K, fl32(fl32(a + b) / 2) of the two middle values for even K.
 * The rule is unweighted: every client has one vote, whatever its sample count.  bf16 rows are
 * widened exactly and the result is fp32, as on the bf16 wire.
 *
 * Conventions (those of fedagg_mx4.h)
 *   - d_* are device pointers owned by the caller; the pointer table is a host array, read before
 *     the call returns.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream); the call is asynchronous on it,
 *     allocates nothing and never synchronises the host, so it may be captured into a graph.
 *   - Every argument is checked before the first HIP call: a refused call has launched nothing.
 *     Return: 0, or a negative code with fedagg_robust_last_error() giving the calling thread's
 *     message.  M == 0 returns FEDAGG_OK and touches nothing.
 */
#ifndef FEDAGG_ROBUST_H
#define FEDAGG_ROBUST_H

#include <stddef.h>
#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FEDAGG_ROBUST_ABI_VERSION 1
#define FEDAGG_ROBUST_MAX_K 128 /* clients: all K values of an element are held in registers at once */

int fedagg_robust_abi_version(void);
const char* fedagg_robust_last_error(void);

/* The sizes at which the kernel changes path.  A lane of the vector walk owns up to *vec_f32
 * consecutive elements of fp32 rows and *vec_bf16 of bf16 rows (the counts up to 32 clients; they
 * halve at 33..64 and again at 65..128 clients, where the registers hold more values per element),
 * and a workgroup step covers up to *tile_elems elements.  The elements past the last whole lane,
 * and every element of a call whose rows or d_out are not 16-B aligned, go one per lane.  Any
 * pointer may be NULL. */
int fedagg_robust_blocking(int* tile_elems, int* vec_f32, int* vec_bf16);

/* The trimmed mean of the rule above over K rows of M elements of `kind` (FEDAGG_F32, or FEDAGG_BF16
 * widened exactly; any other kind is FEDAGG_EINVAL): M fp32 to d_out.  d_rows is a host table of K
 * device addresses.  Rows need their element's alignment and d_out 4 B; rows that are all 16-B
 * aligned together with a 16-B aligned d_out take the vector walk, anything else one element per
 * lane, with identical bits.  d_out must not overlap a row.
 * FEDAGG_EINVAL, each with its own text: K <= 0 or K > FEDAGG_ROBUST_MAX_K, t < 0 or 2 t >= K, a bad
 * kind, a NULL d_rows, row or d_out, a row not aligned to its element, d_out not 4-B aligned. */
int fedagg_robust_mean(const void* const* d_rows, int kind, int K, int t, uint64_t M, float* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDAGG_ROBUST_H */
