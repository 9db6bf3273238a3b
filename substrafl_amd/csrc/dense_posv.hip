// dense_posv.hip -- libfedagg_dense.so: what the Cholesky route of NewtonRaphson's Newton system
// needs next to fedagg_dense_potrf_f64 (include/fedagg_dense.h), for gfx950:
//   dense_flag_clear        *flag = 0, one thread,
//   dense_symcopy_f64       the symmetry test of A by value, with the copy of its lower triangle: a
//                           workgroup per pair of DN_TM x DN_TM tiles (bi, bj), (bj, bi), bi >= bj;
//                           the upper one goes through LDS so that both are read along rows,
//   dense_potrs_fwd_f64     L y = b, the step of one block of DN_NB rows (dense.hip's dense_fwd_f64 with
//                           the factor's own diagonal),
//   dense_potrs_bwd_f64     L^T x = y, the step of one block: a thread per COLUMN of L, so that the
//                           rows of the block finished last are read along rows.
// The stream orders the kernels; no kernel waits on another workgroup, no sum uses an atomic, and no
// index or trip count depends on a matrix value.
#include "dense_internal.h"

static_assert(DN_TM == DN_TN, "the symmetry test pairs square tiles");
static_assert(DN_NB <= 64, "one wave solves a block's triangle");

using namespace fedagg_dense_detail;

namespace {

#define DN_SS (DN_TM + 1)  // row stride of the transposed tile: odd, a column read is 2 per bank pair

__global__ void dense_flag_clear(int32_t* flag) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *flag = 0;
}

// Workgroup b of the 1-D grid takes the tile pair (bi, bj), bi >= bj, rows first: b = bi (bi + 1) / 2 + bj
// (the numbering of dense_potrf_update_f64).  The upper tile (bj, bi) is read along its rows into sU;
// the lower tile (bi, bj) is then read along its rows, element (r, c) against sU[c][r].  A diagonal
// tile meets itself: its diagonal elements are compared with themselves, which only a NaN fails.
// Every thread that sees a mismatch stores the constant 1: the same value whoever wins.
__global__ __launch_bounds__(DN_BLOCK) void dense_symcopy_f64(const double* A, dn_u64 n, dn_u64 lda, double* L, dn_u64 ldl,
                                                              int32_t* flag) {
  __shared__ double sU[DN_TM][DN_SS];
  const int t = threadIdx.x;
  const unsigned b = blockIdx.x;
  unsigned bi = (unsigned)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
  while ((dn_u64)bi * (bi + 1) / 2 > b) --bi;
  while ((dn_u64)(bi + 1) * (bi + 2) / 2 <= b) ++bi;
  const unsigned bj = b - (unsigned)((dn_u64)bi * (bi + 1) / 2);
  const dn_u64 i0 = (dn_u64)bi * DN_TM, j0 = (dn_u64)bj * DN_TM;
  for (int e = t; e < DN_TM * DN_TM; e += DN_BLOCK) {
    const int r = e / DN_TM, c = e % DN_TM;  // of the upper tile: row j0 + r, column i0 + c
    if (j0 + (dn_u64)r < n && i0 + (dn_u64)c < n) sU[r][c] = A[(j0 + (dn_u64)r) * lda + i0 + (dn_u64)c];
  }
  __syncthreads();
  bool differs = false;
  for (int e = t; e < DN_TM * DN_TM; e += DN_BLOCK) {
    const int r = e / DN_TM, c = e % DN_TM;  // of the lower tile: row i0 + r, column j0 + c
    const dn_u64 gr = i0 + (dn_u64)r, gc = j0 + (dn_u64)c;
    if (gr < n && gc <= gr) {  // (gc <= gr < n: the mirrored element was loaded)
      const double v = A[gr * lda + gc];
      if (!(v == sU[c][r])) differs = true;
      if (L) L[gr * ldl + gc] = v;
    }
  }
  if (differs) *flag = 1;
}

// Forward substitution with L, the step of block jb (rows [jb, jb + bs)): every row i >= jb takes off
// the previous block's finished y (L[i][jb-32 .. jb) . y, k ascending); rows past this block are
// written back, this block's rows stay in wave 0 of workgroup 0, which solves the lower triangle
// L11 (with its diagonal: a division per row) from LDS and writes y in place.
__global__ __launch_bounds__(DN_BLOCK) void dense_potrs_fwd_f64(const double* Lf, dn_u64 n, dn_u64 ldl, double* b, dn_u64 jb) {
  __shared__ double sx[DN_NB];
  __shared__ double sT[DN_NB][DN_NB + 1];
  const int t = threadIdx.x;
  const int bs = panel_width(n, jb);
  const bool has_prev = jb > 0;
  const dn_u64 prev = jb - DN_NB;
  if (has_prev && t < DN_NB) sx[t] = b[prev + (dn_u64)t];
  if (blockIdx.x == 0) load_diag_block(sT, Lf, ldl, jb, t, [bs](int r, int k) { return k <= r && r < bs; });
  __syncthreads();
  const dn_u64 i = jb + (dn_u64)blockIdx.x * DN_BLOCK + (dn_u64)t;
  double ri = 0.0;
  if (i < n) {
    ri = b[i];
    if (has_prev) {
      const double* row = Lf + i * ldl + prev;
#pragma unroll
      for (int k = 0; k < DN_NB; ++k) ri = fma(-row[k], sx[k], ri);
      if (i >= jb + DN_NB) b[i] = ri;
    }
  }
  if (blockIdx.x == 0 && t < 64) {
    for (int k = 0; k < bs; ++k) {
      if (t == k) ri = ri / sT[k][k];
      const double yk = __shfl(ri, k);
      if (t > k && t < bs) ri = fma(-sT[t][k], yk, ri);
    }
    if (t < bs) b[jb + (dn_u64)t] = ri;
  }
}

// Back substitution with L^T, the step of block jb, from the last block up: thread q of the grid takes
// COLUMN c = jb + bs - 1 - q of L (row c of L^T) and takes off sum_r L[r][c] x[r] over the rows r of
// the block below, finished by the launch before (r ascending).  For one r the threads of a wave read
// neighbouring elements of row r; no thread walks down a column.  Columns left of this block are
// written back; wave 0 of workgroup 0 keeps this block's and solves L11^T (element (r, k) of it is
// L11[k][r], k >= r) from LDS.
__global__ __launch_bounds__(DN_BLOCK) void dense_potrs_bwd_f64(const double* Lf, dn_u64 n, dn_u64 ldl, double* b, dn_u64 jb) {
  __shared__ double sx[DN_NB];
  __shared__ double sT[DN_NB][DN_NB + 1];
  const int t = threadIdx.x;
  const int bs = panel_width(n, jb);
  const dn_u64 prev = jb + DN_NB;
  const bool has_prev = prev < n;
  const int pbs = has_prev ? panel_width(n, prev) : 0;
  if (t < DN_NB) sx[t] = t < pbs ? b[prev + (dn_u64)t] : 0.0;
  if (blockIdx.x == 0) load_diag_block(sT, Lf, ldl, jb, t, [bs](int r, int k) { return k <= r && r < bs; });
  __syncthreads();
  const dn_u64 top = jb + (dn_u64)bs - 1;
  const dn_u64 q = (dn_u64)blockIdx.x * DN_BLOCK + (dn_u64)t;
  double ri = 0.0;
  if (q <= top) {
    const dn_u64 c = top - q;
    ri = b[c];
    if (has_prev) {
      const double* col = Lf + prev * ldl + c;  // rows prev .. prev + pbs of column c < prev: below the diagonal
      for (int k = 0; k < pbs; ++k) ri = fma(-col[(dn_u64)k * ldl], sx[k], ri);
      if (c < jb) b[c] = ri;
    }
  }
  if (blockIdx.x == 0 && t < 64) {
    const int r = bs - 1 - t;  // this lane's row of the block (negative: none)
    for (int kk = bs - 1; kk >= 0; --kk) {
      if (r == kk) ri = ri / sT[kk][kk];
      const double xk = __shfl(ri, bs - 1 - kk);
      if (r >= 0 && r < kk) ri = fma(-sT[kk][r], xk, ri);
    }
    if (r >= 0) b[jb + (dn_u64)r] = ri;
  }
}

int launch_symcopy(const double* A, dn_u64 n, dn_u64 lda, double* L, dn_u64 ldl, int32_t* flag, hipStream_t st) {
  dense_flag_clear<<<1, 64, 0, st>>>(flag);
  const dn_u64 tiles = (n + DN_TM - 1) / DN_TM;  // <= 2^14: tiles (tiles + 1) / 2 fits a grid
  dense_symcopy_f64<<<(unsigned)(tiles * (tiles + 1) / 2), DN_BLOCK, 0, st>>>(A, n, lda, L, ldl, flag);
  return check_launch("fedagg_dense_symcopy_f64");
}

int launch_potrs(const double* L, dn_u64 n, dn_u64 ldl, double* b, hipStream_t st) {
  for (dn_u64 jb = 0; jb < n; jb += DN_NB) dense_potrs_fwd_f64<<<blocks_for(n - jb), DN_BLOCK, 0, st>>>(L, n, ldl, b, jb);
  for (dn_u64 jb = (n - 1) / DN_NB * DN_NB;; jb -= DN_NB) {
    dense_potrs_bwd_f64<<<blocks_for(jb + (dn_u64)panel_width(n, jb)), DN_BLOCK, 0, st>>>(L, n, ldl, b, jb);
    if (jb == 0) break;
  }
  return check_launch("fedagg_dense_potrs_f64");
}

// Bytes from the first to behind the last element of n rows of leading dimension ld (n >= 1, checked).
inline dn_u64 span_bytes(dn_u64 n, dn_u64 ld) { return ((n - 1) * ld + n) * 8; }

}  // namespace

extern "C" {

int fedagg_dense_symcopy_f64(const double* d_A, uint64_t n, uint64_t lda, double* d_L, uint64_t ldl, int32_t* d_flag,
                             void* stream) {
  if (n == 0) return FEDAGG_DENSE_OK;
  if (int rc = check_matrix(d_A, n, lda)) return rc;
  if (!d_flag) return fail(FEDAGG_DENSE_EINVAL, "d_flag is NULL");
  if (d_L) {
    if (int rc = check_ld("ldl", ldl, "n", n, n)) return rc;
    const uintptr_t a = (uintptr_t)d_A, l = (uintptr_t)d_L;
    if (a < l + span_bytes(n, ldl) && l < a + span_bytes(n, lda)) return fail(FEDAGG_DENSE_EINVAL, "d_L overlaps d_A");
  }
  return launch_symcopy(d_A, n, lda, d_L, d_L ? ldl : 0, d_flag, (hipStream_t)stream);
}

int fedagg_dense_potrs_f64(const double* d_L, uint64_t n, uint64_t ldl, double* d_b, void* stream) {
  if (n == 0) return FEDAGG_DENSE_OK;
  if (!d_L) return fail(FEDAGG_DENSE_EINVAL, "d_L is NULL");
  if (int rc = check_dim("n", n)) return rc;
  if (int rc = check_ld("ldl", ldl, "n", n, n)) return rc;
  if (!d_b) return fail(FEDAGG_DENSE_EINVAL, "d_b is NULL");
  return launch_potrs(d_L, n, ldl, d_b, (hipStream_t)stream);
}

}  // extern "C"
