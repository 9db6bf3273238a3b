// dense_posv.hip -- libfedagg_dense.so: what the Cholesky route of NewtonRaphson's Newton system
// needs next to fedagg_dense_potrf_f64 (include/fedagg_dense.h), for gfx950:
//   dense_flag_clear        *flag = 0, one thread,
//   dense_symcopy_f64       the symmetry test of A by value, with the copy of its lower triangle: a
//                           workgroup per pair of DN_TM x DN_TM tiles (bi, bj), (bj, bi), bi >= bj;
//                           the upper one goes through LDS so that both are read along rows,
//   dense_potrs_fwd_f64     L y = b, the step of one block of DN_NB rows,
//   dense_potrs_bwd_f64     L^T x = y, the step of one block: both are the substitution step of
//                           dense_internal.h, which the LU's solve in dense.hip instantiates too.
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

// Workgroup b of the 1-D grid takes the tile pair (bi, bj), bi >= bj, rows first (lower_tile, the numbering
// of dense_potrf_update_f64).  The upper tile (bj, bi) is read along its rows into sU;
// the lower tile (bi, bj) is then read along its rows, element (r, c) against sU[c][r].  A diagonal
// tile meets itself: its diagonal elements are compared with themselves, which only a NaN fails.
// Every thread that sees a mismatch stores the constant 1: the same value whoever wins.
__global__ __launch_bounds__(DN_BLOCK) void dense_symcopy_f64(const double* A, dn_u64 n, dn_u64 lda, double* L, dn_u64 ldl,
                                                              int32_t* flag) {
  __shared__ double sU[DN_TM][DN_SS];
  const int t = threadIdx.x;
  unsigned bi, bj;
  lower_tile(blockIdx.x, &bi, &bj);
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

// The substitution steps of dense_internal.h for L L^T x = b: L with its own diagonal, L^T read as L's columns.
__global__ __launch_bounds__(DN_BLOCK) void dense_potrs_fwd_f64(const double* Lf, dn_u64 n, dn_u64 ldl, double* b, dn_u64 jb) {
  subst_fwd_step<false>(Lf, n, ldl, b, jb);
}

__global__ __launch_bounds__(DN_BLOCK) void dense_potrs_bwd_f64(const double* Lf, dn_u64 n, dn_u64 ldl, double* b, dn_u64 jb) {
  subst_bwd_step<true>(Lf, n, ldl, b, jb);
}

int launch_symcopy(const double* A, dn_u64 n, dn_u64 lda, double* L, dn_u64 ldl, int32_t* flag, hipStream_t st) {
  dense_flag_clear<<<1, 64, 0, st>>>(flag);
  const dn_u64 tiles = (n + DN_TM - 1) / DN_TM;  // <= 2^14: tiles (tiles + 1) / 2 fits a grid
  dense_symcopy_f64<<<(unsigned)(tiles * (tiles + 1) / 2), DN_BLOCK, 0, st>>>(A, n, lda, L, ldl, flag);
  return check_launch("fedagg_dense_symcopy_f64");
}

int launch_potrs(const double* L, dn_u64 n, dn_u64 ldl, double* b, hipStream_t st) {
  launch_subst(dense_potrs_fwd_f64, dense_potrs_bwd_f64, L, n, ldl, b, st);
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
  if (int rc = check_ptr(d_flag, "d_flag")) return rc;
  if (d_L) {
    if (int rc = check_ld("ldl", ldl, "n", n, n)) return rc;
    const uintptr_t a = (uintptr_t)d_A, l = (uintptr_t)d_L;
    if (a < l + span_bytes(n, ldl) && l < a + span_bytes(n, lda)) return fail(FEDAGG_DENSE_EINVAL, "d_L overlaps d_A");
  }
  return launch_symcopy(d_A, n, lda, d_L, d_L ? ldl : 0, d_flag, (hipStream_t)stream);
}

int fedagg_dense_potrs_f64(const double* d_L, uint64_t n, uint64_t ldl, double* d_b, void* stream) {
  if (n == 0) return FEDAGG_DENSE_OK;
  if (int rc = check_ptr(d_L, "d_L")) return rc;
  if (int rc = check_dim("n", n)) return rc;
  if (int rc = check_ld("ldl", ldl, "n", n, n)) return rc;
  if (int rc = check_ptr(d_b, "d_b")) return rc;
  return launch_potrs(d_L, n, ldl, d_b, (hipStream_t)stream);
}

}  // extern "C"
