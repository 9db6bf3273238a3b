// dense.hip -- libfedagg_dense.so: in-place fp64 LU with partial pivoting and a one right-hand-side
// solve for gfx950 (include/fedagg_dense.h).  A blocked right-looking factorisation: per block
// column of DN_NB columns
//   dense_panel_f64    one workgroup factors the block column (pivot search, row swap inside the
//                      panel, scale, rank-1 updates),
//   dense_laswp_f64    the panel's row interchanges on the columns left and right of it,
//   dense_trsm_f64     U12 = L11^-1 A12 (one thread per column, L11 from LDS),
//   dense_update_f64   A22 -= L21 U12, DN_TM x DN_TN tiles (the tile step of dense_internal.h),
// then dense_perm_f64 and, per block of DN_NB rows, dense_fwd_f64 / dense_bwd_f64 (the substitution
// step of dense_internal.h) for the right-hand side.  The stream orders the kernels; no kernel waits
// on another workgroup, and no sum uses an atomic.
#include "dense_internal.h"

// The panel kernel's blocking.  DN_NB is dense_internal.h's: the strides below are multiples of it, and the suite
// reads all four from this file, so it is stated here once more; a value other than the header's does not compile.
#pragma clang diagnostic push
#pragma clang diagnostic error "-Wmacro-redefined"
#define DN_NB 32
#pragma clang diagnostic pop
#define DN_PANEL_THREADS 512  // the panel kernel's one workgroup: DN_NB columns x DN_RG row groups
#define DN_RG (DN_PANEL_THREADS / 32)
#define DN_UB 8                // rows a panel thread keeps in flight per step of the rank-1 update

using namespace fedagg_dense_detail;

namespace {

// (value, row) candidates of the pivot search: the larger value wins, the smaller row on a tie,
// so the result is the first row of largest |a| whatever the order of the reduction.
__device__ __forceinline__ void pivot_better(double& v, dn_u64& i, double ov, dn_u64 oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// Factor columns [j, j + nb) of rows [j, n), unblocked and right-looking, in global memory (the
// panel of a large matrix does not fit LDS; its rows stay in L2).  Thread t works on panel column
// t & 31 of the rows (t >> 5) + DN_RG k in the rank-1 update (a row's 32 doubles: one 256-B access
// per half wave) and on row t + DN_PANEL_THREADS k in the strided passes over one column (search,
// scale).
// The search of column c + 1 rides on the update of column c.
__global__ __launch_bounds__(DN_PANEL_THREADS) void dense_panel_f64(double* A, dn_u64 n, dn_u64 lda, dn_u64 j, int nb,
                                                                    int32_t* ipiv, int32_t* info) {
  __shared__ double s_v[DN_PANEL_THREADS / 64];
  __shared__ dn_u64 s_i[DN_PANEL_THREADS / 64];
  __shared__ dn_u64 s_piv;
  __shared__ int s_zero;
  const dn_u64 t = threadIdx.x;
  const int col = (int)(t & 31);
  const dn_u64 rg = t >> 5;
  const dn_u64 pc = j + (dn_u64)col;
  if (j == 0 && t == 0) *info = 0;

  // column 0 of the panel: a pass of its own
  double bv = -1.0;
  dn_u64 bi = j;
#pragma unroll 4
  for (dn_u64 i = j + t; i < n; i += DN_PANEL_THREADS) {
    const double v = fabs(A[i * lda + j]);
    if (v > bv) {
      bv = v;
      bi = i;
    }
  }

  for (int c = 0; c < nb; ++c) {
    const dn_u64 jc = j + (dn_u64)c;
    // ---- reduce the candidates (bv, bi) of every thread to the pivot row
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_down(bv, off);
      const dn_u64 oi = __shfl_down(bi, off);
      pivot_better(bv, bi, ov, oi);
    }
    if ((t & 63) == 0) {
      s_v[t >> 6] = bv;
      s_i[t >> 6] = bi;
    }
    __syncthreads();
    if (t == 0) {
      double v = s_v[0];
      dn_u64 p = s_i[0];
      for (int w = 1; w < DN_PANEL_THREADS / 64; ++w) pivot_better(v, p, s_v[w], s_i[w]);
      ipiv[jc] = (int32_t)p;
      const int zero = v == 0.0;
      if (zero && *info == 0) *info = (int32_t)(jc + 1);
      s_piv = p;
      s_zero = zero;
    }
    __syncthreads();
    const dn_u64 p = s_piv;
    const int zero = s_zero;
    // ---- interchange rows jc and p inside the panel
    if (p != jc && col < nb && rg == 0) {
      const double a = A[jc * lda + pc], b = A[p * lda + pc];
      A[jc * lda + pc] = b;
      A[p * lda + pc] = a;
    }
    __syncthreads();
    // ---- scale the column below the pivot (a zero pivot: left as it is, as LAPACK does)
    if (!zero) {
      const double piv = A[jc * lda + jc];
      for (dn_u64 i0 = jc + 1 + t; i0 < n; i0 += 4 * DN_PANEL_THREADS) {
        double a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const dn_u64 i = i0 + (dn_u64)q * DN_PANEL_THREADS;
          a[q] = i < n ? A[i * lda + jc] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const dn_u64 i = i0 + (dn_u64)q * DN_PANEL_THREADS;
          if (i < n) A[i * lda + jc] = a[q] / piv;
        }
      }
    }
    __syncthreads();
    // ---- rank-1 update of the panel's columns right of c; column c + 1's candidates on the way
    bv = -1.0;
    bi = jc + 1;
    if (col > c && col < nb) {
      const bool track = col == c + 1;
      const double u = A[jc * lda + pc];
      for (dn_u64 i0 = jc + 1 + rg; i0 < n; i0 += DN_RG * DN_UB) {
        double l[DN_UB], v[DN_UB];
#pragma unroll
        for (int q = 0; q < DN_UB; ++q) {
          const dn_u64 i = i0 + DN_RG * (dn_u64)q;
          l[q] = i < n ? A[i * lda + jc] : 0.0;
          v[q] = i < n ? A[i * lda + pc] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < DN_UB; ++q) {
          const dn_u64 i = i0 + DN_RG * (dn_u64)q;
          if (i < n) {
            const double r = fma(-l[q], u, v[q]);
            A[i * lda + pc] = r;
            if (track && fabs(r) > bv) {
              bv = fabs(r);
              bi = i;
            }
          }
        }
      }
    }
    __syncthreads();
  }
}

// The panel's interchanges (rows j + c <-> ipiv[j + c], c ascending) on every column outside the
// panel: one thread per column, so a wave moves contiguous pieces of two rows.
__global__ __launch_bounds__(DN_BLOCK) void dense_laswp_f64(double* A, dn_u64 n, dn_u64 lda, dn_u64 j, int nb,
                                                            const int32_t* ipiv) {
  __shared__ dn_u64 s_p[DN_NB];
  if (threadIdx.x < (unsigned)nb) s_p[threadIdx.x] = (dn_u64)(uint32_t)ipiv[j + threadIdx.x];
  __syncthreads();
  const dn_u64 q = (dn_u64)blockIdx.x * DN_BLOCK + threadIdx.x;
  if (q >= n - (dn_u64)nb) return;
  const dn_u64 col = q < j ? q : q + (dn_u64)nb;
  for (int c = 0; c < nb; ++c) {
    const dn_u64 r = j + (dn_u64)c, p = s_p[c];
    if (p != r && p < n) {
      const double a = A[r * lda + col], b = A[p * lda + col];
      A[r * lda + col] = b;
      A[p * lda + col] = a;
    }
  }
}

// U12 = L11^-1 A12 for a full panel (DN_NB rows): one thread per column right of the panel, its
// DN_NB values in registers, the unit lower triangle L11 broadcast from LDS.
__global__ __launch_bounds__(DN_BLOCK) void dense_trsm_f64(double* A, dn_u64 n, dn_u64 lda, dn_u64 j) {
  __shared__ double sL[DN_NB][DN_NB + 1];
  load_diag_block(sL, A, lda, j, threadIdx.x, [](int r, int k) { return k < r; });
  __syncthreads();
  const dn_u64 col = j + DN_NB + (dn_u64)blockIdx.x * DN_BLOCK + threadIdx.x;
  if (col >= n) return;
  double x[DN_NB];
#pragma unroll
  for (int r = 0; r < DN_NB; ++r) x[r] = A[(j + (dn_u64)r) * lda + col];
#pragma unroll
  for (int r = 1; r < DN_NB; ++r) {
    double s = x[r];
#pragma unroll
    for (int k = 0; k < r; ++k) s = fma(-sL[r][k], x[k], s);
    x[r] = s;
  }
#pragma unroll
  for (int r = 1; r < DN_NB; ++r) A[(j + (dn_u64)r) * lda + col] = x[r];
}

// A22 -= L21 U12 below and right of a full panel.  A workgroup takes a DN_TM x DN_TN tile of A22:
// -L21's 64 x 32 and U12's 32 x 64 pieces go through LDS, each wave holds a 32 x 32 quarter seeded
// with A22 itself.  Rows and columns past n: zeros in LDS, their accumulator entries never stored.
__global__ __launch_bounds__(DN_BLOCK) void dense_update_f64(double* A, dn_u64 n, dn_u64 lda, dn_u64 j) {
  __shared__ double sL[DN_TM][DN_LS];
  __shared__ double sU[DN_NB][DN_US];
  const int t = threadIdx.x;
  const dn_u64 r0 = j + DN_NB + (dn_u64)blockIdx.y * DN_TM;
  const dn_u64 c0 = j + DN_NB + (dn_u64)blockIdx.x * DN_TN;
  for (int e = t; e < DN_TM * DN_NB; e += DN_BLOCK) {
    const int r = e / DN_NB, k = e % DN_NB;
    sL[r][k] = r0 + (dn_u64)r < n ? -A[(r0 + (dn_u64)r) * lda + j + (dn_u64)k] : 0.0;
  }
  for (int e = t; e < DN_NB * DN_TN; e += DN_BLOCK) {
    const int k = e / DN_TN, c = e % DN_TN;
    sU[k][c] = c0 + (dn_u64)c < n ? A[(j + (dn_u64)k) * lda + c0 + (dn_u64)c] : 0.0;
  }
  __syncthreads();
  const TileLane ln = quarter_lane(t);
  dn_f64x4 acc[2][2];
  DN_EACH_ACC(2, 2) {
    const dn_u64 r = r0 + (dn_u64)ln.row(mi, q), c = c0 + (dn_u64)ln.col(ni);
    acc[mi][ni][q] = (r < n && c < n) ? A[r * lda + c] : 0.0;
  }
  tile_step(acc, ln, sL, [&](int k, int c) { return sU[k][c]; });
  DN_EACH_ACC(2, 2) {
    const dn_u64 r = r0 + (dn_u64)ln.row(mi, q), c = c0 + (dn_u64)ln.col(ni);
    if (r < n && c < n) A[r * lda + c] = acc[mi][ni][q];
  }
}

// b <- P b: the interchanges in order, by one thread (each may depend on the one before).
__global__ void dense_perm_f64(const int32_t* ipiv, dn_u64 n, double* b) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (dn_u64 r = 0; r < n; ++r) {
    const dn_u64 p = (dn_u64)(uint32_t)ipiv[r];
    if (p != r && p < n) {
      const double a = b[r], c = b[p];
      b[r] = c;
      b[p] = a;
    }
  }
}

// The substitution steps of dense_internal.h for L U x = P b: L has ones on its diagonal, U is read along rows.
__global__ __launch_bounds__(DN_BLOCK) void dense_fwd_f64(const double* LU, dn_u64 n, dn_u64 lda, double* b, dn_u64 jb) {
  subst_fwd_step<true>(LU, n, lda, b, jb);
}

__global__ __launch_bounds__(DN_BLOCK) void dense_bwd_f64(const double* LU, dn_u64 n, dn_u64 lda, double* b, dn_u64 jb) {
  subst_bwd_step<false>(LU, n, lda, b, jb);
}

int launch_getrf(double* A, dn_u64 n, dn_u64 lda, int32_t* ipiv, int32_t* info, hipStream_t st) {
  for (dn_u64 j = 0; j < n; j += DN_NB) {
    const int nb = panel_width(n, j);
    dense_panel_f64<<<1, DN_PANEL_THREADS, 0, st>>>(A, n, lda, j, nb, ipiv, info);
    if (n > (dn_u64)nb) dense_laswp_f64<<<blocks_for(n - nb), DN_BLOCK, 0, st>>>(A, n, lda, j, nb, ipiv);
    if (j + nb < n) {  // a trailing matrix: the panel is a full one
      const dn_u64 rest = n - j - DN_NB;
      dense_trsm_f64<<<blocks_for(rest), DN_BLOCK, 0, st>>>(A, n, lda, j);
      const dim3 grid((unsigned)((rest + DN_TN - 1) / DN_TN), (unsigned)((rest + DN_TM - 1) / DN_TM));
      dense_update_f64<<<grid, DN_BLOCK, 0, st>>>(A, n, lda, j);
    }
  }
  return check_launch("fedagg_dense_getrf_f64");
}

int launch_getrs(const double* LU, dn_u64 n, dn_u64 lda, const int32_t* ipiv, double* b, hipStream_t st) {
  dense_perm_f64<<<1, 64, 0, st>>>(ipiv, n, b);
  launch_subst(dense_fwd_f64, dense_bwd_f64, LU, n, lda, b, st);
  return check_launch("fedagg_dense_getrs_f64");
}

}  // namespace

extern "C" {

int fedagg_dense_abi_version(void) { return FEDAGG_DENSE_ABI_VERSION; }

const char* fedagg_dense_last_error(void) { return g_error; }

int fedagg_dense_blocking(int* panel, int* tile_m, int* tile_n) {
  if (!panel || !tile_m || !tile_n) return fail(FEDAGG_DENSE_EINVAL, "fedagg_dense_blocking: NULL output pointer");
  *panel = DN_NB;
  *tile_m = DN_TM;
  *tile_n = DN_TN;
  return FEDAGG_DENSE_OK;
}

uint64_t fedagg_dense_ws_bytes(uint64_t n) {
  (void)n;  // the factorisation works in place: the panel, the triangle and the tiles live in LDS
  return 0;
}

int fedagg_dense_getrf_f64(double* d_A, uint64_t n, uint64_t lda, int32_t* d_ipiv, int32_t* d_info, void* d_ws,
                           void* stream) {
  (void)d_ws;
  if (n == 0) return FEDAGG_DENSE_OK;
  if (int rc = check_matrix(d_A, n, lda)) return rc;
  if (int rc = check_ptr(d_ipiv, "d_ipiv")) return rc;
  if (int rc = check_ptr(d_info, "d_info")) return rc;
  return launch_getrf(d_A, n, lda, d_ipiv, d_info, (hipStream_t)stream);
}

int fedagg_dense_getrs_f64(const double* d_LU, uint64_t n, uint64_t lda, const int32_t* d_ipiv, double* d_b,
                           void* stream) {
  if (n == 0) return FEDAGG_DENSE_OK;
  if (int rc = check_matrix(d_LU, n, lda)) return rc;
  if (int rc = check_ptr(d_ipiv, "d_ipiv")) return rc;
  if (int rc = check_ptr(d_b, "d_b")) return rc;
  return launch_getrs(d_LU, n, lda, d_ipiv, d_b, (hipStream_t)stream);
}

int fedagg_dense_solve_f64(double* d_A, uint64_t n, uint64_t lda, int32_t* d_ipiv, int32_t* d_info, double* d_b,
                           void* d_ws, void* stream) {
  (void)d_ws;
  if (n == 0) return FEDAGG_DENSE_OK;
  if (int rc = check_matrix(d_A, n, lda)) return rc;
  if (int rc = check_ptr(d_ipiv, "d_ipiv")) return rc;
  if (int rc = check_ptr(d_info, "d_info")) return rc;
  if (int rc = check_ptr(d_b, "d_b")) return rc;
  if (int rc = launch_getrf(d_A, n, lda, d_ipiv, d_info, (hipStream_t)stream)) return rc;
  return launch_getrs(d_A, n, lda, d_ipiv, d_b, (hipStream_t)stream);
}

}  // extern "C"
