/*
 * fedagg_dense.h -- C ABI of libfedagg_dense.so: a dense fp64 LU solve on MI355X (gfx950) for
 * NewtonRaphson's Newton system (substrafl/strategies/newton_raphson.py:213,
 * `np.linalg.solve(total_hessians, total_gradient_one_d)`), and a dense fp64 Cholesky
 * factorisation for its clients' Hessian check (torch_newton_raphson_algo.py:346-352).
 *
 * A library of its own beside libfedagg.so: nothing in fedagg.h changes, and the aggregation
 * engine loads this one only when a caller opts in (integration.accelerate(..., solve="device")).
 * The default stays the reference's host solve, bit for bit.
 *
 * Accuracy contract (u = 2^-53, gamma_n = n u / (1 - n u)).  Unlike fedagg.h, nothing here is
 * bit-identical to NumPy: a device LU cannot reproduce LAPACK's rounding, and LAPACK's own bits
 * differ between BLAS builds.  What is promised instead:
 *   - partial pivoting: at step j the pivot is the first row i >= j of largest |a_ij|, so every
 *     multiplier satisfies |l_ij| <= 1;
 *   - the factors satisfy the componentwise bound |P A - L U| <= gamma_n |L| |U| (Higham, Accuracy
 *     and Stability of Numerical Algorithms, thm 9.3: any summation order, with or without FMA);
 *   - for matrices whose growth factor is of order 1 the solution's normwise backward error
 *     ||b - A x||inf / (||A||inf ||x||inf + ||b||inf) is at most n u (tests/test_dense_solve_gpu.py);
 *   - the Cholesky factor of fedagg_dense_potrf_f64 satisfies |A - L L^T| <= gamma_{n+1} |L| |L^T|
 *     on the lower triangle (Higham thm 10.3: any summation order, with or without FMA; fp64
 *     sqrt and division are correctly rounded), so a run that ends with *d_info == 0 proves A + E
 *     positive definite for an E within that bound (tests/test_dense_potrf_gpu.py);
 *   - the solution of fedagg_dense_potrs_f64 from that computed L satisfies the componentwise bound
 *     |b - A x| <= gamma_{3n+1} |L| |L^T| |x| (Higham thm 10.4: any summation order, with or without
 *     FMA), and on the positive definite families of tests/test_dense_posv_gpu.py the normwise
 *     backward error above is at most n u;
 *   - the Householder LQ of fedagg_dense_gelqf_f64 / fedagg_dense_orglq_f64 (A = L Q, n <= m; LAPACK's
 *     dgelqf + dorglq arithmetic with dlarfg's sign, beta = -sign(alpha) ||(alpha, x)||, so Q is
 *     np.linalg.qr(A.T)[0].T with no sign fix-up): the relative residual ||A - L Q||_F / ||A||_2 and
 *     the loss of orthogonality ||Q Q^T - I||_F are each at most m n u sqrt(n) (Higham thm 19.4 and
 *     19.13 with constant 1: any summation order, with or without FMA) and at most
 *     max(4 x LAPACK's own value, 8 u sqrt(n)) on the inputs of tests/test_dense_lq_gpu.py.  A
 *     rank-deficient A still gives orthonormal rows (an all-zero row tail is tau = 0, H = I).
 *     Norms are plain fp64 sums of squares: an A whose squares overflow or underflow fp64 is
 *     outside the contract (a widened fp32 matrix never is);
 *   - results are deterministic: the same build gives the same bits on every run and stream
 *     (no atomics, every sum in a fixed order -- for the LQ an order fixed by (n, m) alone;
 *     contraction to FMA is allowed).
 * Inputs with NaN or Inf raise nothing and fault nothing; their outputs are unspecified.
 *
 * Conventions (those of fedagg.h)
 *   - d_* are device pointers owned by the caller; matrices are ROW-major with a leading dimension
 *     of lda >= n ELEMENTS; elements [n, lda) of a row are never read or written.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream); every call is asynchronous on
 *     it, allocates nothing and never synchronises the host: the launch sequence is a function of
 *     n alone, the kernels are ordered by the stream alone.
 *   - Every argument is checked before the first HIP call.  Return: 0, or a negative code with
 *     fedagg_dense_last_error() giving the calling thread's message.
 *   - n == 0 returns FEDAGG_DENSE_OK and touches nothing.
 */
#ifndef FEDAGG_DENSE_H
#define FEDAGG_DENSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FEDAGG_DENSE_ABI_VERSION 1
#define FEDAGG_DENSE_MAX_N (1u << 20) /* an 8 TiB matrix: beyond any HBM, keeps every grid in range */

enum {
  FEDAGG_DENSE_OK = 0,
  FEDAGG_DENSE_EINVAL = -1, /* bad argument (NULL pointer, lda < n, size overflow, ...) */
  FEDAGG_DENSE_EHIP = -2,   /* a HIP runtime call failed                                */
};

int fedagg_dense_abi_version(void);
const char* fedagg_dense_last_error(void);

/* The blocking the kernels use: `panel` columns are factored at a time (also the block of the
 * triangular solves and of the substitutions), the trailing update works on tile_m x tile_n
 * tiles.  Sizes next to these and their multiples are where the kernels change path. */
int fedagg_dense_blocking(int* panel, int* tile_m, int* tile_n);

/* Bytes of device workspace fedagg_dense_getrf_f64 / fedagg_dense_solve_f64 need for order n
 * (may be 0: d_ws may then be NULL). */
uint64_t fedagg_dense_ws_bytes(uint64_t n);

/* In-place LU with partial pivoting, P A = L U (blocked, right-looking; the trailing update on
 * v_mfma_f64_16x16x4_f64).  L is unit lower triangular, stored below the diagonal; U on and
 * above it.  d_ipiv[j] (0-based, in [j, n)) is the row interchanged with row j at step j.
 * *d_info is 0, or j + 1 for the first exactly-zero pivot u_jj: the factorisation then goes on
 * as LAPACK's does (no fault), and what it leaves in d_A is unspecified. */
int fedagg_dense_getrf_f64(double* d_A, uint64_t n, uint64_t lda, int32_t* d_ipiv, int32_t* d_info, void* d_ws,
                           void* stream);

/* Solve A x = b from the factors of fedagg_dense_getrf_f64, one right-hand side, in place in d_b:
 * the interchanges, then blocked forward (L) and back (U) substitution. */
int fedagg_dense_getrs_f64(const double* d_LU, uint64_t n, uint64_t lda, const int32_t* d_ipiv, double* d_b,
                           void* stream);

/* fedagg_dense_getrf_f64 then fedagg_dense_getrs_f64.  With *d_info != 0 afterwards d_b holds
 * unspecified values (divisions by the zero pivot), as d_A does. */
int fedagg_dense_solve_f64(double* d_A, uint64_t n, uint64_t lda, int32_t* d_ipiv, int32_t* d_info, double* d_b,
                           void* d_ws, void* stream);

/* In-place lower Cholesky, A = L L^T (blocked, right-looking; the trailing update on
 * v_mfma_f64_16x16x4_f64 over the tiles on and below the diagonal).  Only elements with row >=
 * column are read, and L is written there: the strict upper triangle, like elements [n, lda) of a
 * row, is never read or written.  Needs no workspace.
 * *d_info is 0 -- the certificate that A (its lower triangle mirrored) is positive definite to
 * within the backward error above -- or j + 1 for the first pivot d = a_jj - sum_k l_jk^2 that is
 * not > 0 (a NaN counts, as in LAPACK's dpotrf) or is +Inf.  The factorisation then goes on, on
 * whatever values there are (no fault): rows and columns [0, j) of L, the leading triangle, are
 * the factor's, everything else in the lower triangle is unspecified. */
int fedagg_dense_potrf_f64(double* d_A, uint64_t n, uint64_t lda, int32_t* d_info, void* stream);

/* ---- Householder LQ of an n x m matrix, n <= m (added within ABI version 1) ----
 * Here a matrix has n rows of m elements, lda >= m (ldq >= m); elements [m, lda) of a row are
 * never read or written, and the launch sequence is a function of (n, m) alone.  n > m, n or m
 * above FEDAGG_DENSE_MAX_N, lda < m, ldq < m and a NULL pointer (d_ws included: the workspace is
 * never empty for n >= 1) are refused with FEDAGG_DENSE_EINVAL. */

/* The blocking of the LQ kernels: `panel` rows are factored at a time, the block reflector works
 * on tile_m x tile_n tiles, and W = C V^T is reduced over chunks of k_chunk columns. */
int fedagg_dense_lq_blocking(int* panel, int* tile_m, int* tile_n, int* k_chunk);

/* Bytes of device workspace either call below needs for an n x m matrix (0 for n == 0). */
uint64_t fedagg_dense_lq_ws_bytes(uint64_t n, uint64_t m);

/* A (n x m, n <= m, lda >= m) = L Q in place (blocked, right-looking, compact-WY block reflectors
 * on v_mfma_f64_16x16x4_f64): L on and below the diagonal of the first n columns, reflector j,
 * H_j = I - tau_j v_j^T v_j, in row j right of the diagonal (unit element implied), d_tau[j].  A row
 * tail that is all zero gives tau_j = 0 and leaves a_jj as it is, sign included (always so for
 * j = n - 1 when n == m). */
int fedagg_dense_gelqf_f64(double* d_A, uint64_t n, uint64_t m, uint64_t lda, double* d_tau, void* d_ws, void* stream);

/* The n x m Q with orthonormal rows (== np.linalg.qr(A.T)[0].T), from gelqf's output (d_A and d_tau
 * are only read), into d_Q: the first n rows of the identity times H_k ... H_1, the block reflectors
 * rebuilt from d_A and d_tau alone.  d_ws need not be the one gelqf used. */
int fedagg_dense_orglq_f64(const double* d_A, uint64_t n, uint64_t m, uint64_t lda, const double* d_tau, double* d_Q,
                           uint64_t ldq, void* d_ws, void* stream);

/* ---- The solve from a Cholesky factor and the symmetry test ahead of it (added within ABI version 1) ----
 * For a Newton system that is symmetric positive definite: symcopy (is it symmetric? and a copy of its
 * lower triangle, A itself stays intact), fedagg_dense_potrf_f64 on the copy, potrs.  Square matrices
 * under the conventions above; the leading dimension of a factor is ldl >= n. */

/* *d_flag = 0 if a_ij == a_ji by value for every i >= j, the diagonal included -- np.array_equal(A, A.T):
 * a NaN anywhere is "not symmetric", -0.0 equals 0.0 -- else 1.  If d_L is not NULL, the lower triangle
 * of A (row >= column) is copied into it bit for bit, whatever the flag; the strict upper triangle of
 * d_L and elements [n, ldl) of its rows are never written.  d_A is only read.  d_L = NULL tests only
 * (ldl is then ignored).  A d_L whose n rows overlap those of d_A is refused. */
int fedagg_dense_symcopy_f64(const double* d_A, uint64_t n, uint64_t lda, double* d_L, uint64_t ldl, int32_t* d_flag,
                             void* stream);

/* Solve L L^T x = b from the factor of fedagg_dense_potrf_f64, one right-hand side, in place in d_b:
 * blocked forward (L) and back (L^T) substitution, with divisions by l_kk (no inverted block).  Only
 * elements of d_L with row >= column are read.  After a potrf whose *d_info != 0 the factor is
 * unspecified and so is x. */
int fedagg_dense_potrs_f64(const double* d_L, uint64_t n, uint64_t ldl, double* d_b, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDAGG_DENSE_H */
