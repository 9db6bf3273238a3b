/*
 * fedagg_topk.h -- C ABI of libfedagg_topk.so: the top-k sparse wire of FedAvg on MI355X (gfx950).
 * The client's exact magnitude top-k selection with error feedback and ordered compaction, and the
 * aggregator's FedAvg over K sparse rows into a dense fp32 average without densifying them.
 *
 * A client update on the top-k wire is nnz (index, value) pairs: 4-byte flat indices into the
 * raveled concatenation of the layers, strictly ascending, and the 4-byte fp32 values at them.  At
 * 1 % density that is 0.08 bytes per parameter against 0.53 for MXFP4 (fedagg_mx4.h).  What is not
 * sent stays in the client's fp32 residual (4 bytes per parameter of device memory) and is added
 * to the next round's update.
 *
 * A library of its own beside libfedagg.so and the MX libraries: nothing in their headers changes,
 * and only a top-k call loads it.  The kinds (FEDAGG_F32, FEDAGG_BF16) and the return codes are
 * those of fedagg.h.
 *
 * The rule (all fp32, never contracted; x the flat update widened exactly, res the residual)
 *   r   = fl32(x + res)
 *   m   = bits(r) & 0x7FFFFFFF as uint32: NaN and Inf sort above every finite value
 *   t   = the k-th largest of m over all M elements
 *   kept  every i with m_i >= max(t, 1): every tie at the threshold is kept, so nnz >= k unless
 *         fewer than k elements are non-zero; zeros are never sent, an all-zero r gives nnz == 0
 *   values  the kept r_i, bit for bit, in ascending order of i
 *   res'_i = +0.0 where i is kept or r_i is not finite, r_i elsewhere
 * substrafl_amd/wire.py restates the rule in NumPy (topk_error_feedback); the tests hold the
 * kernels to it bit for bit.
 *
 * Conventions (those of fedagg_mxdl.h)
 *   - d_* are device pointers owned by the caller; the pointer tables, nnz, h_w and h_pw_idx are
 *     host arrays, read before the call returns.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream); every call is asynchronous on
 *     it, allocates nothing and never synchronises the host, so it may be captured into a graph.
 *   - Every argument is checked before the first HIP call: a refused call has launched nothing.
 *     Return: 0, or a negative code with fedagg_topk_last_error() giving the calling thread's
 *     message.  M == 0 returns FEDAGG_OK and touches nothing.  M is below 2^32.
 */
#ifndef FEDAGG_TOPK_H
#define FEDAGG_TOPK_H

#include <stddef.h>
#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FEDAGG_TOPK_ABI_VERSION 1
#define FEDAGG_TOPK_KMAX 128        /* clients per fedavg call (kernel-argument table)            */
#define FEDAGG_TOPK_STATE_WORDS 8   /* uint32 words of d_state                                    */
/* d_state, written by the device: */
#define FEDAGG_TOPK_STATE_T 0       /* t, the k-th largest magnitude pattern                      */
#define FEDAGG_TOPK_STATE_NNZ 1     /* the number of kept elements                                */
#define FEDAGG_TOPK_STATE_ERROR 2   /* 0, or 1 once a compact call's nnz differed from the word above */
/* words 3..7 are the selection's own (threshold, radix prefix, remaining rank) */

int fedagg_topk_abi_version(void);
const char* fedagg_topk_last_error(void);

/* The sizes at which the kernels change path.  Selection and compaction: a workgroup of *threads
 * lanes covers *select_tile consecutive elements per step, a lane four consecutive elements at a
 * time (one 16-B load where d_res, and d_x for its element size, are 16-B aligned and the four lie
 * inside the row; one by one otherwise).  FedAvg: a wave owns *sub_tile consecutive elements of the
 * output in LDS, and clients are loaded *k_group at a time ahead of the in-order add chain (the
 * last K % k_group clients one by one).  Any pointer may be NULL. */
int fedagg_topk_blocking(int* select_tile, int* sub_tile, int* k_group, int* threads);

/* Bytes of d_ws that fedagg_topk_select (and the compact call after it) needs for M elements, and
 * that fedagg_topk_fedavg needs for K rows of M elements.  Either pointer may be NULL.
 * FEDAGG_EINVAL: M at or above 2^32, K outside [0, FEDAGG_TOPK_KMAX]. */
int fedagg_topk_workspace(uint64_t M, int K, size_t* select_bytes, size_t* fedavg_bytes);

/* The selection: an exact radix select on the 31 magnitude bits in three histogram passes of 11,
 * 10 and 10 bits.  Pass 1 is fused: it reads d_x (in_kind FEDAGG_F32, or FEDAGG_BF16 widened
 * exactly) and d_res, forms r and stores r over d_res in place (res' = r wherever nothing is sent),
 * and histograms the top 11 bits in LDS; passes 2 and 3 read d_res only.  Between the passes a
 * one-workgroup kernel fixes the radix prefix and the remaining rank in d_state, so no host round
 * trip separates them.  A count pass and a one-workgroup scan then leave each tile's offset in d_ws
 * and t and nnz in d_state (FEDAGG_TOPK_STATE_WORDS uint32; the error word is cleared).  The only
 * atomics are integer adds into the histograms.
 * FEDAGG_EINVAL, each with its own text: a bad in_kind, M at or above 2^32, k outside [1, M], NULL
 * d_x / d_res / d_ws / d_state, d_x or d_res not aligned to its element, d_ws or d_state not 16-B
 * aligned, d_res overlapping d_x, ws_bytes below fedagg_topk_workspace's select_bytes. */
int fedagg_topk_select(int in_kind, const void* d_x, float* d_res, uint64_t M, uint64_t k, void* d_ws,
                       size_t ws_bytes, uint32_t* d_state, void* stream);

/* The compaction after a selection over the same d_res, M, d_ws and d_state.  nnz is what the caller
 * read from d_state; where it differs from the device's word the kernel writes nothing but the
 * error word.  Each workgroup re-derives the flags of its tile, ranks them with wave ballots and
 * popcounts and one LDS exchange across its waves, and writes the indices (d_idx, nnz uint32) and
 * values (d_val, nnz fp32) at its tile's offset: the row is ascending with no sort.  It stores +0.0
 * at the kept and the non-finite positions of d_res.  nnz == 0 needs no d_idx / d_val.
 * FEDAGG_EINVAL, each with its own text: M at or above 2^32, nnz above M, NULL d_res / d_ws /
 * d_state, NULL d_idx / d_val with nnz > 0, d_res / d_idx / d_val not 4-B aligned. */
int fedagg_topk_compact(float* d_res, uint64_t M, const void* d_ws, uint32_t* d_state, uint64_t nnz, uint32_t* d_idx,
                        float* d_val, void* stream);

/* FedAvg over K sparse rows into the dense average d_out (M fp32): row k is nnz[k] strictly
 * ascending indices below M at d_idx[k] and the values at d_val[k] (either may be NULL where
 * nnz[k] == 0).  For every element, fedagg_fedavg_f32's arithmetic on the densified rows exactly,
 *     acc = +0.0;  for k in 0..K-1 (list order):  acc = fl32(acc + fl32(x_k[i] * h_w[k]))
 * where an absent element contributes fl32(+0 * w) and acc + (+-0) == acc for every acc reachable
 * from +0.0.  A bounds kernel does one lower_bound per client and sub-tile edge into d_ws; the
 * reduce kernel gives each wave a sub-tile in LDS and walks the clients in list order with plain LDS
 * read-modify-writes (a client's indices are unique, a wave's LDS operations retire in program
 * order: no barrier, no atomics); the sub-tile leaves as whole 16-B stores where d_out is 16-B
 * aligned.  The P flat indices in h_pw_idx (numel == 1 layers; may be NULL when P == 0) take
 *     out = +0.0 + pairwise_sum(p_0 .. p_{K-1})
 * with NumPy's pairwise tree instead, absent terms as fl32(+0 * w), in a second small kernel.
 * Rows whose indices are not ascending or not below M give an unspecified average, never an access
 * outside d_out: the caller checks its rows (wire.topk_check).
 * FEDAGG_EINVAL, each with its own text: K outside [1, FEDAGG_TOPK_KMAX], M at or above 2^32, NULL
 * d_idx / d_val / nnz / h_w / d_ws / d_out, nnz[k] above M, a NULL or misaligned row with
 * nnz[k] > 0, d_out not 4-B aligned, P < 0, NULL h_pw_idx with P > 0, an index >= M, ws_bytes below
 * fedagg_topk_workspace's fedavg_bytes. */
int fedagg_topk_fedavg(const uint32_t* const* d_idx, const float* const* d_val, const uint64_t* nnz, const float* h_w,
                       int K, uint64_t M, const uint64_t* h_pw_idx, int P, void* d_ws, size_t ws_bytes, float* d_out,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDAGG_TOPK_H */
