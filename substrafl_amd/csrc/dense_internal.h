// dense_internal.h -- what the sources of libfedagg_dense.so share: the blocking, the calling
// thread's error message, the argument checks every entry point makes before its first HIP call,
// and the device code more than one factorisation or solve uses: the 32 x 32 block load, the triangular
// grid decode, the substitution step of the LU and Cholesky solves, and the MFMA tile step of the updates.
#ifndef FEDAGG_DENSE_INTERNAL_H
#define FEDAGG_DENSE_INTERNAL_H

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "fedagg_dense.h"

#define DN_NB 32      // panel width; block of the triangular solves and substitutions
#define DN_TM 64      // trailing-update tile, rows
#define DN_TN 64      // trailing-update tile, columns
#define DN_BLOCK 256
#define DN_LS (DN_NB + 4)   // row stride of a [row][k] image: 4 (mod 32) doubles, the 64 operand reads 2 per bank
#define DN_US (DN_TN + 16)  // row stride of a [k][col] B image: 16 (mod 32) doubles, likewise

typedef double dn_f64x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long dn_u64;

namespace fedagg_dense_detail {

inline thread_local char g_error[256] = "";  // one per thread for the whole library (fedagg_dense_last_error)

__attribute__((format(printf, 2, 3))) inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
  return code;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) return FEDAGG_DENSE_OK;
  snprintf(g_error, sizeof(g_error), "%s: %s", what, hipGetErrorString(e));
  return FEDAGG_DENSE_EHIP;
}

// The pieces of the argument checks, before any HIP call: a pointer that must not be NULL, ...
inline int check_ptr(const void* p, const char* name) {
  if (!p) return fail(FEDAGG_DENSE_EINVAL, "%s is NULL", name);
  return FEDAGG_DENSE_OK;
}

// ... a dimension (named "n" or "m") ...
inline int check_dim(const char* name, uint64_t v) {
  if (v > FEDAGG_DENSE_MAX_N) return fail(FEDAGG_DENSE_EINVAL, "%s = %lld exceeds FEDAGG_DENSE_MAX_N", name, (long long)v);
  return FEDAGG_DENSE_OK;
}

// ... and the leading dimension (named "lda" or "ldq") of n >= 1 rows of `cols` (named "n" or "m") columns.
inline int check_ld(const char* name, uint64_t ld, const char* cols_name, uint64_t cols, uint64_t n) {
  if (ld < cols) return fail(FEDAGG_DENSE_EINVAL, "%s = %lld is smaller than %s", name, (long long)ld, cols_name);
  if (ld > UINT64_MAX / 8 / n)
    return fail(FEDAGG_DENSE_EINVAL, "n * %s * 8 overflows 64 bits (n = %lld)", name, (long long)n);
  return FEDAGG_DENSE_OK;
}

// The argument checks of the square entry points (n >= 1 here).
inline int check_matrix(const void* d_A, uint64_t n, uint64_t lda) {
  if (int rc = check_ptr(d_A, "d_A")) return rc;
  if (int rc = check_dim("n", n)) return rc;
  return check_ld("lda", lda, "n", n, n);
}

inline unsigned blocks_for(dn_u64 work) { return (unsigned)((work + DN_BLOCK - 1) / DN_BLOCK); }

// Width of the panel (rows of the block) that starts at j < n: DN_NB but for the last one.
__host__ __device__ inline int panel_width(dn_u64 n, dn_u64 j) { return (int)(n - j < DN_NB ? n - j : DN_NB); }

// ------------------------------------------------------------------ device code, DN_BLOCK threads
// f(r, k) for every element of a DN_NB x DN_NB block, 4 per thread t, a wave on consecutive k.
template <class F>
__device__ __forceinline__ void each_block_elem(int t, F f) {
  for (int e = t; e < DN_NB * DN_NB; e += DN_BLOCK) f(e / DN_NB, e % DN_NB);
}

// The DN_NB x DN_NB block at (j, j) of A into an LDS image: the elements keep(r, k) holds for, zeros elsewhere
// (which are not read from memory: the last block may be a narrow one).
template <class P>
__device__ __forceinline__ void load_diag_block(double (&s)[DN_NB][DN_NB + 1], const double* A, dn_u64 lda, dn_u64 j, int t,
                                                P keep) {
  each_block_elem(t, [&](int r, int k) { s[r][k] = keep(r, k) ? A[(j + (dn_u64)r) * lda + j + (dn_u64)k] : 0.0; });
}

// Workgroup b of a 1-D grid over the tiles (ty, tx), ty >= tx, of a lower triangle, rows first:
// b = ty (ty + 1) / 2 + tx.  The float root is within one of the answer, the two loops settle it.
__device__ __forceinline__ void lower_tile(unsigned b, unsigned* ty, unsigned* tx) {
  unsigned y = (unsigned)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
  while ((dn_u64)y * (y + 1) / 2 > b) --y;
  while ((dn_u64)(y + 1) * (y + 2) / 2 <= b) ++y;
  *ty = y;
  *tx = b - (unsigned)((dn_u64)y * (y + 1) / 2);
}

// The substitution step: one block of DN_NB rows of a triangular solve with one right-hand side, in place in b.
// A launch per block, in the order of the sweep; the block finished by the launch before is only read, this block
// is read and written by workgroup 0 alone.
//
// Forward, L x = b with the lower triangle of T, the step of block jb (rows [jb, jb + bs)): every row i >= jb
// takes off the previous block's finished x (T[i][jb-32 .. jb) . x, k ascending); rows past this block are
// written back, this block's rows stay in wave 0 of workgroup 0, which solves the triangle L11 from LDS and
// writes x in place.  UNIT_DIAG: L has ones on its diagonal and T's own is not read (the L of an LU); otherwise
// a division per row by T's diagonal (a Cholesky factor).
template <bool UNIT_DIAG>
__device__ __forceinline__ void subst_fwd_step(const double* T, dn_u64 n, dn_u64 ld, double* b, dn_u64 jb) {
  __shared__ double sx[DN_NB];
  __shared__ double sT[DN_NB][DN_NB + 1];
  const int t = threadIdx.x;
  const int bs = panel_width(n, jb);
  const bool has_prev = jb > 0;
  const dn_u64 prev = jb - DN_NB;
  if (has_prev && t < DN_NB) sx[t] = b[prev + (dn_u64)t];
  if (blockIdx.x == 0) load_diag_block(sT, T, ld, jb, t, [bs](int r, int k) { return (UNIT_DIAG ? k < r : k <= r) && r < bs; });
  __syncthreads();
  const dn_u64 i = jb + (dn_u64)blockIdx.x * DN_BLOCK + (dn_u64)t;
  double ri = 0.0;
  if (i < n) {
    ri = b[i];
    if (has_prev) {
      const double* row = T + i * ld + prev;
#pragma unroll
      for (int k = 0; k < DN_NB; ++k) ri = fma(-row[k], sx[k], ri);
      if (i >= jb + DN_NB) b[i] = ri;
    }
  }
  if (blockIdx.x == 0 && t < 64) {
    for (int k = 0; k < bs; ++k) {
      if (!UNIT_DIAG && t == k) ri = ri / sT[k][k];
      const double xk = __shfl(ri, k);
      if (t > k && t < bs) ri = fma(-sT[t][k], xk, ri);
    }
    if (t < bs) b[jb + (dn_u64)t] = ri;
  }
}

// Backward, U x = b with a division per row, the step of block jb from the last block up, the mirror image:
// thread q of the grid takes row i = jb + bs - 1 - q of U, takes off the block below-right's finished x
// (k ascending), rows above this block are written back, and wave 0 of workgroup 0 solves the triangle U11 for
// this block's rows.  U is the upper triangle of T, read along T's rows; or, TRANSPOSED, U = L^T for the lower
// triangle L of T (a Cholesky factor): row i of U is COLUMN i of T, so for one k the threads of a wave read
// neighbouring elements of T's row prev + k and no thread walks down a column, and element (r, k) of U11 is
// L11[k][r].
template <bool TRANSPOSED>
__device__ __forceinline__ void subst_bwd_step(const double* T, dn_u64 n, dn_u64 ld, double* b, dn_u64 jb) {
  __shared__ double sx[DN_NB];
  __shared__ double sT[DN_NB][DN_NB + 1];
  const int t = threadIdx.x;
  const int bs = panel_width(n, jb);
  const dn_u64 prev = jb + DN_NB;
  const bool has_prev = prev < n;
  const int pbs = has_prev ? panel_width(n, prev) : 0;
  if (t < DN_NB) sx[t] = t < pbs ? b[prev + (dn_u64)t] : 0.0;
  if (blockIdx.x == 0)
    load_diag_block(sT, T, ld, jb, t, [bs](int r, int k) { return TRANSPOSED ? k <= r && r < bs : k >= r && k < bs; });
  __syncthreads();
  const dn_u64 top = jb + (dn_u64)bs - 1;
  const dn_u64 q = (dn_u64)blockIdx.x * DN_BLOCK + (dn_u64)t;
  double ri = 0.0;
  if (q <= top) {
    const dn_u64 i = top - q;
    ri = b[i];
    if (has_prev) {
      // U[i][prev + k]: TRANSPOSED, rows prev .. prev + pbs of T's column i < prev, below the diagonal
      const double* u = TRANSPOSED ? T + prev * ld + i : T + i * ld + prev;
      for (int k = 0; k < pbs; ++k) ri = fma(-u[TRANSPOSED ? (dn_u64)k * ld : (dn_u64)k], sx[k], ri);
      if (i < jb) b[i] = ri;
    }
  }
  if (blockIdx.x == 0 && t < 64) {
    const int r = bs - 1 - t;  // this lane's row of the block (negative: none)
    for (int kk = bs - 1; kk >= 0; --kk) {
      if (r == kk) ri = ri / sT[kk][kk];
      const double xk = __shfl(ri, bs - 1 - kk);
      if (r >= 0 && r < kk) ri = fma(-(TRANSPOSED ? sT[kk][r] : sT[r][kk]), xk, ri);
    }
    if (r >= 0) b[jb + (dn_u64)r] = ri;
  }
}

// Both sweeps of such a solve on stream st: the forward step for every block from the first down, then the
// backward step for every block from the last up.  Each grid covers the rows its step still touches.
typedef void (*subst_kernel)(const double*, dn_u64, dn_u64, double*, dn_u64);
inline void launch_subst(subst_kernel fwd, subst_kernel bwd, const double* T, dn_u64 n, dn_u64 ld, double* b, hipStream_t st) {
  for (dn_u64 jb = 0; jb < n; jb += DN_NB) fwd<<<blocks_for(n - jb), DN_BLOCK, 0, st>>>(T, n, ld, b, jb);
  for (dn_u64 jb = (n - 1) / DN_NB * DN_NB;; jb -= DN_NB) {
    bwd<<<blocks_for(jb + (dn_u64)panel_width(n, jb)), DN_BLOCK, 0, st>>>(T, n, ld, b, jb);
    if (jb == 0) break;
  }
}

// The tile step: C += A B for a DN_TM x DN_TN (or narrower) tile of C and DN_NB k-values, on
// v_mfma_f64_16x16x4_f64.  A workgroup is 4 waves; a wave holds MI x NI accumulators of 16 x 16 whose
// top left corner is (wm, wn) in the tile.  The instruction's maps, for lane l of the wave:
//   operand A   one double, A[row = l & 15][k = l >> 4],
//   operand B   one double, B[k = l >> 4][col = l & 15],
//   C/D         four doubles, register q is C[row = (l >> 4) + 4 q][col = l & 15].
// The sign convention of every caller: the negated operand goes into LDS and the accumulators are
// seeded with the target, so the step only ever adds.
struct TileLane {
  int l15, l4;  // l & 15, l >> 4
  int wm, wn;   // the wave's origin in the tile
  __device__ __forceinline__ int row(int mi, int q) const { return wm + mi * 16 + l4 + 4 * q; }  // of acc[mi][.][q]
  __device__ __forceinline__ int col(int ni) const { return wn + ni * 16 + l15; }                // of acc[.][ni][.]
};

// The 2 x 2 grid of 32 x 32 quarters of the three trailing updates: wave w at (w >> 1, w & 1).
__device__ __forceinline__ TileLane quarter_lane(int t) { return {t & 15, (t & 63) >> 4, (t >> 7) * 32, ((t >> 6) & 1) * 32}; }

// The four 16-row strips of a 64 x 32 tile (dense_lq_wpart_f64): wave w at rows 16 w.
__device__ __forceinline__ TileLane strip_lane(int t) { return {t & 15, (t & 63) >> 4, (t >> 6) * 16, 0}; }

// The traversal of a wave's MI x NI accumulators: the statement after it runs for every element acc[mi][ni][q],
// which is the tile's (ln.row(mi, q), ln.col(ni)); the macro declares mi, ni and q in that statement's scope.
// A macro over plain loops, not a functor: with the body in a lambda the
// compiler forms every element's address on its own instead of per column, 120 more instructions per update kernel
// and 0.6 to 2.9 % of its time on an MI355X (profiles/dense_tile_refactor.log).
#define DN_PRAGMA_UNROLL _Pragma("unroll")
#define DN_EACH_ACC(MI, NI)                                                   \
  DN_PRAGMA_UNROLL for (int mi = 0; mi < (MI); ++mi)                          \
    DN_PRAGMA_UNROLL for (int ni = 0; ni < (NI); ++ni)                        \
      DN_PRAGMA_UNROLL for (int q = 0; q < 4; ++q)

// The DN_NB / 4 k-steps.  A from a [row][k] image of the tile's rows; B through b_at(k, tile column), so a
// [k][col] image (stride DN_US) and a [col][k] image (stride DN_LS) both fit.
template <int MI, int NI, class B>
__device__ __forceinline__ void tile_step(dn_f64x4 (&acc)[MI][NI], const TileLane& ln, const double (*sA)[DN_LS], B b_at) {
#pragma unroll
  for (int ks = 0; ks < DN_NB / 4; ++ks) {
    double a[MI], b[NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) a[mi] = sA[ln.wm + mi * 16 + ln.l15][ks * 4 + ln.l4];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) b[ni] = b_at(ks * 4 + ln.l4, ln.wn + ni * 16 + ln.l15);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
  }
}

}  // namespace fedagg_dense_detail

#endif  // FEDAGG_DENSE_INTERNAL_H
