/*
 * fedagg_krum.h -- C ABI of libfedagg_krum.so: the fp64 Gram matrix G = X X^T of K client rows, the
 * device half of Krum and multi-Krum (Blanchard et al. 2017), on MI355X (gfx950).
 *
 * The coordinate-wise rules of fedagg_robust.h look at one element at a time: a client whose update is
 * unremarkable in every coordinate but wrong as a vector (sign-flipped, scaled into the honest range,
 * colluding) passes them.  Krum selects whole clients by their pairwise distances
 * d_ij = G_ii + G_jj - 2 G_ij, and every one of them comes from the K x K matrix of inner products of
 * the rows: a very skinny GEMM, K <= 128 and M in the hundreds of millions, that reads K M elements
 * once and runs on the matrix units (v_mfma_f64_16x16x4_f64).  The selection itself is a few lines on
 * the host (substrafl_amd.engine.krum_select).
 *
 * A library of its own beside libfedagg.so and the other satellite libraries: nothing in their
 * headers changes, and only a Krum call loads it.  The kinds (FEDAGG_F32, FEDAGG_BF16) and the
 * return codes are those of fedagg.h.
 *
 * Arithmetic.  Every element is widened to fp64 exactly; every product of two widened values is
 * exact in fp64 (24 + 24 bits for fp32 rows, 8 + 8 for bf16); only the additions round.  The order
 * of the additions is a function of (K, M, kind) alone: two calls give the same bits, whatever the
 * device does meanwhile and however the rows are aligned.  The result is held to an error bound,
 *   |G^_ij - G_ij| <= gamma_M (|X| |X|^T)_ij,   gamma_M = M u / (1 - M u),   u = 2^-53,
 * which holds for any order because the products are exact; it is not held to NumPy's bits.  A NaN
 * or Inf of client i reaches row i and column i of G and nothing else.
 *
 * Conventions (those of fedagg_robust.h)
 *   - d_* are device pointers owned by the caller; the pointer table is a host array, read before
 *     the call returns.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream); the call is asynchronous on it,
 *     allocates nothing and never synchronises the host, so it may be captured into a graph.
 *   - Every argument is checked before the first HIP call: a refused call has launched nothing.
 *     Return: 0, or a negative code with fedagg_krum_last_error() giving the calling thread's
 *     message.
 *   - M == 0 is the empty sum: the K x K zero matrix (+0.0) is written to d_G.  The checks are the
 *     same as for any M (fedagg_krum_ws_bytes gives 0 bytes, d_ws must still be a valid pointer).
 */
#ifndef FEDAGG_KRUM_H
#define FEDAGG_KRUM_H

#include <stddef.h>
#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FEDAGG_KRUM_ABI_VERSION 1
#define FEDAGG_KRUM_MAX_K 128 /* clients: 8 blocks of 16, 36 tiles of 16 x 16 in the upper triangle */

int fedagg_krum_abi_version(void);
const char* fedagg_krum_last_error(void);

/* The sizes at which the kernel changes path: a workgroup step covers *chunk_elems elements of every
 * row, and a lane loads *vec_f32 consecutive elements of an fp32 row or *vec_bf16 of a bf16 row per
 * step (16 B).  The last elements of a row that do not fill a lane's 16 B, and every element of a call
 * whose rows are not all 16-B aligned, are loaded one at a time into the same places: identical bits.
 * Any pointer may be NULL. */
int fedagg_krum_blocking(int* chunk_elems, int* vec_f32, int* vec_bf16);

/* Bytes of workspace fedagg_krum_gram needs for K rows of M elements: one partial upper triangle per
 * workgroup, and the number of workgroups is a function of (K, M) alone.  0 for M == 0.
 * FEDAGG_EINVAL: K outside [1, FEDAGG_KRUM_MAX_K], M above 2^44, bytes NULL. */
int fedagg_krum_ws_bytes(int K, uint64_t M, uint64_t* bytes);

/* G[i*K + j] = sum_m x_i[m] * x_j[m] in fp64, the full symmetric K x K matrix (both triangles
 * written, bit-equal), rows of FEDAGG_F32 or FEDAGG_BF16 widened exactly.  d_rows is a host table of K
 * device addresses of M elements each.  Two launches: every workgroup reduces a fixed contiguous
 * share of M into its partial triangle in d_ws, a second kernel adds the partials in workgroup order
 * and writes d_G.  Nothing outside the K*K doubles of d_G and the first fedagg_krum_ws_bytes bytes of
 * d_ws is written; d_ws holds nothing of use afterwards.
 * FEDAGG_EINVAL, each with its own text: K outside [1, FEDAGG_KRUM_MAX_K], a bad kind, a NULL d_rows,
 * row, d_G or d_ws, a row not aligned to its element, d_G not 8-B aligned, d_ws not 16-B aligned,
 * ws_bytes below fedagg_krum_ws_bytes(K, M), M above 2^44. */
int fedagg_krum_gram(const void* const* d_rows, int kind, int K, uint64_t M, void* d_ws, uint64_t ws_bytes,
                     double* d_G, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDAGG_KRUM_H */
