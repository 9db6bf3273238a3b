// dense_potrf.hip -- libfedagg_dense.so: in-place fp64 lower Cholesky, A = L L^T, for gfx950
// (include/fedagg_dense.h: the certificate of NewtonRaphson's Hessian check).  A blocked
// right-looking factorisation that reads and writes the lower triangle only: per block column of
// DN_NB columns
//   dense_potrf_diag_f64    one workgroup factors the diagonal block in LDS and records the first
//                           pivot that is not > 0,
//   dense_potrf_panel_f64   L21 = A21 L11^-T (one thread per row, L11 from LDS),
//   dense_potrf_update_f64  A22 -= L21 L21^T, the DN_TM x DN_TN tiles on and below the diagonal
//                           only (the tile step of dense_internal.h).
// The stream orders the kernels; no kernel waits on another workgroup, no sum uses an atomic, and
// no index or trip count depends on a matrix value: after a failed pivot everything still runs,
// on whatever values (NaN) there are.
#include "dense_internal.h"

static_assert(DN_TM == DN_TN, "the trailing update walks square tiles on and below the diagonal");
static_assert(DN_TM % DN_NB == 0, "a tile row starts on a panel boundary");

using namespace fedagg_dense_detail;

namespace {

// Factor the nb x nb diagonal block at (j, j), right-looking, in LDS: per column c the pivot
// d = a_cc - sum_k l_ck^2 (the sum already taken off by the steps before), l_cc = sqrt(d), the
// column below it divided by l_cc, then the rank-1 update of the columns right of c.  !(d > 0)
// also holds for a NaN, as in LAPACK's dpotrf; a pivot of +Inf fails as well (its square root
// would zero the column below it and let the rest pass: no certificate of anything).  The first
// such pivot of the whole factorisation stays in *info (the launch of j = 0 writes it
// unconditionally, so the caller need not clear it).
__global__ __launch_bounds__(DN_BLOCK) void dense_potrf_diag_f64(double* A, dn_u64 lda, dn_u64 j, int nb, int32_t* info) {
  __shared__ double s[DN_NB][DN_NB + 1];
  const int t = threadIdx.x;
  load_diag_block(s, A, lda, j, t, [nb](int r, int k) { return k <= r && r < nb; });
  __syncthreads();
  int32_t first = 0;  // thread 0's: 1-based index of the block's first failed pivot
  for (int c = 0; c < nb; ++c) {
    const double d = s[c][c];
    if (t == 0 && (!(d > 0.0) || isinf(d)) && first == 0) first = (int32_t)(j + (dn_u64)c + 1);
    const double l = sqrt(d);
    __syncthreads();  // every thread has read d
    if (t == c) s[c][c] = l;
    if (t > c && t < nb) s[t][c] = s[t][c] / l;
    __syncthreads();
    for (int e = t; e < DN_NB * DN_NB; e += DN_BLOCK) {
      const int r = e / DN_NB, k = e % DN_NB;
      if (k > c && k <= r && r < nb) s[r][k] = fma(-s[r][c], s[k][c], s[r][k]);
    }
    __syncthreads();
  }
  for (int e = t; e < DN_NB * DN_NB; e += DN_BLOCK) {
    const int r = e / DN_NB, k = e % DN_NB;
    if (k <= r && r < nb) A[(j + (dn_u64)r) * lda + j + (dn_u64)k] = s[r][k];
  }
  if (t == 0) {
    if (j == 0)
      *info = first;
    else if (first != 0 && *info == 0)
      *info = first;
  }
}

// L21 = A21 L11^-T below a full diagonal block (DN_NB columns): one thread per row, its DN_NB
// values in registers, the lower triangle L11 (with its diagonal) broadcast from LDS; column k of
// the row is (a_ik - sum_{m<k} l_im l_km) / l_kk, m ascending.
__global__ __launch_bounds__(DN_BLOCK) void dense_potrf_panel_f64(double* A, dn_u64 n, dn_u64 lda, dn_u64 j) {
  __shared__ double sL[DN_NB][DN_NB + 1];
  load_diag_block(sL, A, lda, j, threadIdx.x, [](int r, int k) { return k <= r; });
  __syncthreads();
  const dn_u64 row = j + DN_NB + (dn_u64)blockIdx.x * DN_BLOCK + threadIdx.x;
  if (row >= n) return;
  double* a = A + row * lda + j;
  double x[DN_NB];
#pragma unroll
  for (int k = 0; k < DN_NB; ++k) x[k] = a[k];
#pragma unroll
  for (int k = 0; k < DN_NB; ++k) {
    double v = x[k];
#pragma unroll
    for (int m = 0; m < k; ++m) v = fma(-x[m], sL[k][m], v);
    x[k] = v / sL[k][k];
  }
#pragma unroll
  for (int k = 0; k < DN_NB; ++k) a[k] = x[k];
}

// A22 -= L21 L21^T below and right of a full diagonal block, the lower triangle only.  Workgroup
// b of the 1-D grid takes tile (ty, tx) of the tiles with ty >= tx, rows first (lower_tile).
// Each wave holds a 32 x 32 quarter seeded with A22; both operands are rows of L21, so both
// LDS images are [row][k]: -L21's rows of the tile's rows and L21's rows of the tile's columns.
// Rows past n: zeros in LDS, never stored.  Only entries with row >= column are seeded from and
// stored to A; a quarter wholly above the diagonal (wave 1 of a diagonal tile) does nothing.
__global__ __launch_bounds__(DN_BLOCK) void dense_potrf_update_f64(double* A, dn_u64 n, dn_u64 lda, dn_u64 j) {
  __shared__ double sA[DN_TM][DN_LS];
  __shared__ double sB[DN_TN][DN_LS];
  const int t = threadIdx.x;
  unsigned ty, tx;
  lower_tile(blockIdx.x, &ty, &tx);
  const dn_u64 r0 = j + DN_NB + (dn_u64)ty * DN_TM;
  const dn_u64 c0 = j + DN_NB + (dn_u64)tx * DN_TN;
  for (int e = t; e < DN_TM * DN_NB; e += DN_BLOCK) {  // (one loop for both images: their loads are in flight together)
    const int r = e / DN_NB, k = e % DN_NB;
    sA[r][k] = r0 + (dn_u64)r < n ? -A[(r0 + (dn_u64)r) * lda + j + (dn_u64)k] : 0.0;
    sB[r][k] = c0 + (dn_u64)r < n ? A[(c0 + (dn_u64)r) * lda + j + (dn_u64)k] : 0.0;
  }
  __syncthreads();
  const TileLane ln = quarter_lane(t);
  if (ty == tx && ln.wn > ln.wm) return;  // (after the last barrier)
  dn_f64x4 acc[2][2];
  DN_EACH_ACC(2, 2) {
    const dn_u64 r = r0 + (dn_u64)ln.row(mi, q), c = c0 + (dn_u64)ln.col(ni);
    acc[mi][ni][q] = (r < n && c <= r) ? A[r * lda + c] : 0.0;
  }
  tile_step(acc, ln, sA, [&](int k, int c) { return sB[c][k]; });
  DN_EACH_ACC(2, 2) {
    const dn_u64 r = r0 + (dn_u64)ln.row(mi, q), c = c0 + (dn_u64)ln.col(ni);
    if (r < n && c <= r) A[r * lda + c] = acc[mi][ni][q];
  }
}

int launch_potrf(double* A, dn_u64 n, dn_u64 lda, int32_t* info, hipStream_t st) {
  for (dn_u64 j = 0; j < n; j += DN_NB) {
    const int nb = panel_width(n, j);
    dense_potrf_diag_f64<<<1, DN_BLOCK, 0, st>>>(A, lda, j, nb, info);
    if (j + nb < n) {  // rows below the block: the block is a full one
      const dn_u64 rest = n - j - DN_NB;
      dense_potrf_panel_f64<<<blocks_for(rest), DN_BLOCK, 0, st>>>(A, n, lda, j);
      const dn_u64 tiles = (rest + DN_TM - 1) / DN_TM;  // <= 2^14: tiles (tiles + 1) / 2 fits a grid
      dense_potrf_update_f64<<<(unsigned)(tiles * (tiles + 1) / 2), DN_BLOCK, 0, st>>>(A, n, lda, j);
    }
  }
  return check_launch("fedagg_dense_potrf_f64");
}

}  // namespace

extern "C" int fedagg_dense_potrf_f64(double* d_A, uint64_t n, uint64_t lda, int32_t* d_info, void* stream) {
  if (n == 0) return FEDAGG_DENSE_OK;
  if (int rc = check_matrix(d_A, n, lda)) return rc;
  if (int rc = check_ptr(d_info, "d_info")) return rc;
  return launch_potrf(d_A, n, lda, d_info, (hipStream_t)stream);
}
