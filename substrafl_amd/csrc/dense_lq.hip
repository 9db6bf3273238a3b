// dense_lq.hip -- libfedagg_dense.so: fp64 Householder LQ of a row-major n x m matrix (n <= m),
// A = L Q, and the explicit Q with orthonormal rows, for gfx950 (include/fedagg_dense.h: the
// orthonormalisation of FedPCA's averaged state, np.linalg.qr(a.T)[0].T).  Every Householder
// vector is a contiguous row of A, so nothing is transposed.  A blocked right-looking
// factorisation with compact-WY block reflectors, H_1 .. H_nb = I - V^T T V: per panel of DN_NB rows
//   dense_lq_panel_f64   one workgroup factors rows [j, j + nb), columns [j, m) in global memory
//                        (dlarfg's rule per row, then a dot product and an axpy per remaining row),
//   dense_lq_wpart_f64   W = C V^T, one workgroup per (DN_TM rows, LQ_KC columns): partial products
//                        into the workspace; with C = V itself the same kernel gives the partials
//                        of V V^T,
//   dense_lq_t_f64       V V^T summed in chunk order, then T (upper triangular) from it and tau,
//   dense_lq_wt_f64      W summed in chunk order and multiplied by T (T^T for orglq),
//   dense_lq_apply_f64   C -= (W T) V on DN_TM x DN_TN tiles
// (both products are the tile step of dense_internal.h).
// orglq starts from the first n rows of the identity (dense_lq_eye_f64) and applies the block
// reflectors in reverse order with T^T, T rebuilt from V and tau.  The stream orders the kernels;
// no kernel waits on another workgroup, no sum uses an atomic, every sum runs in an order fixed
// by (n, m), and no index or trip count depends on a matrix value.
#include "dense_internal.h"

#define LQ_KC 512                  // columns one workgroup of dense_lq_wpart_f64 reduces over
#define LQ_PANEL_THREADS 1024      // the panel kernel's one workgroup
#define LQ_PW (LQ_PANEL_THREADS / 64)

static_assert(LQ_KC % DN_NB == 0, "a chunk is a whole number of 32-column steps");

using namespace fedagg_dense_detail;

namespace {

// Element (i, c) of the block's V: row j + i of A with zeros left of its diagonal and the implied
// unit on it; zero past the block's nb rows and past column m.
__device__ __forceinline__ double lq_v(const double* __restrict__ A, dn_u64 lda, dn_u64 j, int nb, int i, dn_u64 c,
                                       dn_u64 m) {
  if (i >= nb || c >= m) return 0.0;
  const dn_u64 d = j + (dn_u64)i;
  return c < d ? 0.0 : c == d ? 1.0 : A[d * lda + c];
}

// Every lane gets the wave's sum: the butterfly adds the same pairs in every lane.
__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}

// Factor rows [j, j + nb) over columns [j, m), unblocked, in global memory (a panel of 32 rows of a
// wide matrix does not fit LDS; it stays in L2).  Per row r: the plain fp64 sum of squares of the
// tail (r, m), strided over the workgroup and reduced in wave order; LAPACK dlarfg's rule by
// thread 0 -- beta = -sign(alpha) sqrt(alpha^2 + |x|^2), tau = (beta - alpha) / beta, the tail times
// 1 / (alpha - beta); an all-zero tail: tau = 0 and the row stays as it is --; then wave w applies
// the reflector to rows r + 1 + w, r + 1 + w + LQ_PW, ... of the panel: w = c_r + c . v, c -= tau w v.
__global__ __launch_bounds__(LQ_PANEL_THREADS) void dense_lq_panel_f64(double* A, dn_u64 m, dn_u64 lda, dn_u64 j, int nb,
                                                                      double* tau) {
  __shared__ double s_part[LQ_PW];
  __shared__ double s_tau, s_scale;
  const dn_u64 t = threadIdx.x;
  const dn_u64 lane = t & 63, w = t >> 6;
  for (int c = 0; c < nb; ++c) {
    const dn_u64 r = j + (dn_u64)c;
    double* __restrict__ row = A + r * lda;
    double ss = 0.0;
#pragma unroll 4
    for (dn_u64 k = r + 1 + t; k < m; k += LQ_PANEL_THREADS) {
      const double x = row[k];
      ss = fma(x, x, ss);
    }
    ss = wave_sum(ss);
    if (lane == 0) s_part[w] = ss;
    __syncthreads();
    if (t == 0) {
      double x2 = s_part[0];
      for (int q = 1; q < LQ_PW; ++q) x2 += s_part[q];
      double tc = 0.0, sc = 0.0;
      if (x2 != 0.0) {
        const double alpha = row[r];
        const double beta = -copysign(sqrt(fma(alpha, alpha, x2)), alpha);
        tc = (beta - alpha) / beta;
        sc = 1.0 / (alpha - beta);
        row[r] = beta;
      }
      tau[r] = tc;
      s_tau = tc;
      s_scale = sc;
    }
    __syncthreads();
    const double tc = s_tau, sc = s_scale;
    if (tc != 0.0) {  // (uniform: tau == 0 is H = I, nothing to scale or apply)
#pragma unroll 4
      for (dn_u64 k = r + 1 + t; k < m; k += LQ_PANEL_THREADS) row[k] = row[k] * sc;
      __syncthreads();
      for (dn_u64 i = r + 1 + w; i < j + (dn_u64)nb; i += LQ_PW) {
        double* __restrict__ ci = A + i * lda;
        double s = 0.0;
#pragma unroll 4
        for (dn_u64 k = r + 1 + lane; k < m; k += 64) s = fma(ci[k], row[k], s);
        const double tw = tc * (ci[r] + wave_sum(s));
#pragma unroll 4
        for (dn_u64 k = r + 1 + lane; k < m; k += 64) ci[k] = fma(-tw, row[k], ci[k]);
        if (lane == 0) ci[r] = ci[r] - tw;
      }
    }
    __syncthreads();
  }
}

// part[chunk][lr][0 .. 32) = sum over the chunk's columns of C[crow0 + lr][c] V[i][c], lr in
// [0, nrows): workgroup (chunk, row tile) walks columns [j + chunk LQ_KC, + LQ_KC) below m in steps
// of 32, both operands through LDS as [row][k]; wave w holds rows 16 w .. 16 w + 15 of the tile as
// two accumulators.  c_is_v: C is V itself (nrows = nb), so the result is the chunk's share of
// V V^T.  Rows past nrows and columns past m: zeros in LDS, never stored.
__global__ __launch_bounds__(DN_BLOCK) void dense_lq_wpart_f64(const double* C, dn_u64 ldc, dn_u64 crow0, dn_u64 nrows,
                                                               int c_is_v, const double* A, dn_u64 lda, dn_u64 j, int nb,
                                                               dn_u64 m, double* part) {
  __shared__ double sC[DN_TM][DN_LS];
  __shared__ double sV[DN_NB][DN_LS];
  const int t = threadIdx.x;
  const dn_u64 chunk = blockIdx.x;
  const dn_u64 r0 = (dn_u64)blockIdx.y * DN_TM;
  const dn_u64 k0 = j + chunk * LQ_KC;
  const dn_u64 k1 = k0 + LQ_KC < m ? k0 + LQ_KC : m;
  const TileLane ln = strip_lane(t);
  dn_f64x4 acc[1][2];
  DN_EACH_ACC(1, 2) acc[mi][ni][q] = 0.0;
  for (dn_u64 kk = k0; kk < k1; kk += DN_NB) {
    for (int e = t; e < DN_TM * DN_NB; e += DN_BLOCK) {
      const int r = e / DN_NB, k = e % DN_NB;
      const dn_u64 lr = r0 + (dn_u64)r, c = kk + (dn_u64)k;
      double v = 0.0;
      if (lr < nrows && c < k1) v = c_is_v ? lq_v(A, lda, j, nb, (int)lr, c, m) : C[(crow0 + lr) * ldc + c];
      sC[r][k] = v;
    }
    for (int e = t; e < DN_NB * DN_NB; e += DN_BLOCK) {
      const int i = e / DN_NB, k = e % DN_NB;
      const dn_u64 c = kk + (dn_u64)k;
      sV[i][k] = c < k1 ? lq_v(A, lda, j, nb, i, c, m) : 0.0;
    }
    __syncthreads();
    tile_step(acc, ln, sC, [&](int k, int i) { return sV[i][k]; });
    __syncthreads();
  }
  DN_EACH_ACC(1, 2) {
    const dn_u64 lr = r0 + (dn_u64)ln.row(mi, q);
    if (lr < nrows) part[(chunk * nrows + lr) * DN_NB + (dn_u64)ln.col(ni)] = acc[mi][ni][q];
  }
}

// T of the block (DN_NB x DN_NB, upper triangular, zeros past nb) from G = V V^T -- its nch partials
// summed in chunk order -- and tau: t_kk = tau_k, T[0..k)[k] = -tau_k T[0..k)[0..k) G[0..k)[k]
// (LAPACK dlarft, forward, rowwise).  One workgroup; thread i owns row i of T.
__global__ __launch_bounds__(DN_BLOCK) void dense_lq_t_f64(const double* part, unsigned nch, int nb, const double* tau,
                                                           double* T) {
  __shared__ double sG[DN_NB][DN_NB + 1];
  __shared__ double sT[DN_NB][DN_NB + 1];
  const int t = threadIdx.x;
  each_block_elem(t, [&](int i, int k) {
    double g = 0.0;
    if (i < nb && k < nb)
      for (unsigned ch = 0; ch < nch; ++ch) g += part[((dn_u64)ch * (dn_u64)nb + (dn_u64)i) * DN_NB + (dn_u64)k];
    sG[i][k] = g;
    sT[i][k] = 0.0;
  });
  __syncthreads();
  for (int k = 0; k < nb; ++k) {
    const double tk = tau[k];
    if (t < k) {
      double s = 0.0;
      for (int l = t; l < k; ++l) s = fma(sT[t][l], sG[l][k], s);
      sT[t][k] = -tk * s;
    } else if (t == k) {
      sT[k][k] = tk;
    }
    __syncthreads();
  }
  for (int e = t; e < DN_NB * DN_NB; e += DN_BLOCK) T[e] = sT[e / DN_NB][e % DN_NB];
}

// W2 = (sum of W's nch partials, in chunk order) T, or ... T^T (trans): thread (row, k) of a
// workgroup's 8 rows sums its element, then takes the row from LDS times column k of T.
__global__ __launch_bounds__(DN_BLOCK) void dense_lq_wt_f64(const double* part, unsigned nch, dn_u64 nrows, const double* T,
                                                            int trans, double* W2) {
  __shared__ double sT[DN_NB][DN_NB + 1];
  __shared__ double sW[DN_BLOCK / DN_NB][DN_NB + 1];
  const int t = threadIdx.x;
  for (int e = t; e < DN_NB * DN_NB; e += DN_BLOCK) {
    const int i = e / DN_NB, k = e % DN_NB;
    if (trans)
      sT[k][i] = T[e];
    else
      sT[i][k] = T[e];
  }
  const int lr = t / DN_NB, k = t % DN_NB;
  const dn_u64 r = (dn_u64)blockIdx.x * (DN_BLOCK / DN_NB) + (dn_u64)lr;
  double s = 0.0;
  if (r < nrows)
    for (unsigned ch = 0; ch < nch; ++ch) s += part[((dn_u64)ch * nrows + r) * DN_NB + (dn_u64)k];
  sW[lr][k] = s;
  __syncthreads();
  double o = 0.0;
#pragma unroll
  for (int i = 0; i < DN_NB; ++i) o = fma(sW[lr][i], sT[i][k], o);
  if (r < nrows) W2[r * DN_NB + (dn_u64)k] = o;
}

// C -= W2 V on rows [crow0, crow0 + nrows), columns [j, m).  A workgroup takes a DN_TM x DN_TN tile:
// -W2's 64 x 32 and V's 32 x 64 pieces go through LDS (V with its unit diagonal and the zeros left
// of it), each wave holds a 32 x 32 quarter seeded with C itself.  Rows past nrows and columns past
// m: zeros in LDS, never loaded or stored.
__global__ __launch_bounds__(DN_BLOCK) void dense_lq_apply_f64(double* C, dn_u64 ldc, dn_u64 crow0, dn_u64 nrows,
                                                               const double* W2, const double* A, dn_u64 lda, dn_u64 j,
                                                               int nb, dn_u64 m) {
  __shared__ double sL[DN_TM][DN_LS];
  __shared__ double sU[DN_NB][DN_US];
  const int t = threadIdx.x;
  const dn_u64 r0 = (dn_u64)blockIdx.y * DN_TM;
  const dn_u64 c0 = j + (dn_u64)blockIdx.x * DN_TN;
  for (int e = t; e < DN_TM * DN_NB; e += DN_BLOCK) {
    const int r = e / DN_NB, k = e % DN_NB;
    sL[r][k] = r0 + (dn_u64)r < nrows ? -W2[(r0 + (dn_u64)r) * DN_NB + (dn_u64)k] : 0.0;
  }
  for (int e = t; e < DN_NB * DN_TN; e += DN_BLOCK) {
    const int k = e / DN_TN, c = e % DN_TN;
    sU[k][c] = lq_v(A, lda, j, nb, k, c0 + (dn_u64)c, m);
  }
  __syncthreads();
  const TileLane ln = quarter_lane(t);
  dn_f64x4 acc[2][2];
  DN_EACH_ACC(2, 2) {
    const dn_u64 lr = r0 + (dn_u64)ln.row(mi, q), c = c0 + (dn_u64)ln.col(ni);
    acc[mi][ni][q] = (lr < nrows && c < m) ? C[(crow0 + lr) * ldc + c] : 0.0;
  }
  tile_step(acc, ln, sL, [&](int k, int c) { return sU[k][c]; });
  DN_EACH_ACC(2, 2) {
    const dn_u64 lr = r0 + (dn_u64)ln.row(mi, q), c = c0 + (dn_u64)ln.col(ni);
    if (lr < nrows && c < m) C[(crow0 + lr) * ldc + c] = acc[mi][ni][q];
  }
}

// Q = the first n rows of the m x m identity (columns [0, m) of every row; [m, ldq) untouched).
__global__ __launch_bounds__(DN_BLOCK) void dense_lq_eye_f64(double* Q, dn_u64 n, dn_u64 m, dn_u64 ldq) {
  const dn_u64 c = (dn_u64)blockIdx.x * DN_BLOCK + threadIdx.x;
  if (c >= m) return;
  for (dn_u64 r = blockIdx.y; r < n; r += gridDim.y) Q[r * ldq + c] = r == c ? 1.0 : 0.0;
}

// The workspace, in doubles: T (DN_NB^2), the partials (chunks x rows x DN_NB, at most
// ceil(m / LQ_KC) x n x DN_NB; V V^T's first, then W's in the same place), W2 (n x DN_NB).
inline dn_u64 chunks_of(dn_u64 cols) { return (cols + LQ_KC - 1) / LQ_KC; }
inline dn_u64 ws_doubles(dn_u64 n, dn_u64 m) { return DN_NB * DN_NB + chunks_of(m) * n * DN_NB + n * DN_NB; }

// The block reflector of rows [j, j + nb) of A on rows [crow0, crow0 + nrows), columns [j, m) of C.
void launch_block(double* C, dn_u64 ldc, dn_u64 crow0, dn_u64 nrows, const double* A, dn_u64 lda, dn_u64 n, dn_u64 m,
                  dn_u64 j, int nb, const double* tau, int trans, double* ws, hipStream_t st) {
  double* T = ws;
  double* part = ws + DN_NB * DN_NB;
  double* W2 = part + chunks_of(m) * n * DN_NB;
  const unsigned nch = (unsigned)chunks_of(m - j);
  const unsigned rt = (unsigned)((nrows + DN_TM - 1) / DN_TM);
  dense_lq_wpart_f64<<<dim3(nch, 1), DN_BLOCK, 0, st>>>(A, lda, j, (dn_u64)nb, 1, A, lda, j, nb, m, part);
  dense_lq_t_f64<<<1, DN_BLOCK, 0, st>>>(part, nch, nb, tau + j, T);
  dense_lq_wpart_f64<<<dim3(nch, rt), DN_BLOCK, 0, st>>>(C, ldc, crow0, nrows, 0, A, lda, j, nb, m, part);
  dense_lq_wt_f64<<<(unsigned)((nrows + DN_BLOCK / DN_NB - 1) / (DN_BLOCK / DN_NB)), DN_BLOCK, 0, st>>>(part, nch, nrows, T,
                                                                                                     trans, W2);
  dense_lq_apply_f64<<<dim3((unsigned)((m - j + DN_TN - 1) / DN_TN), rt), DN_BLOCK, 0, st>>>(C, ldc, crow0, nrows, W2, A, lda,
                                                                                            j, nb, m);
}

int launch_gelqf(double* A, dn_u64 n, dn_u64 m, dn_u64 lda, double* tau, double* ws, hipStream_t st) {
  for (dn_u64 j = 0; j < n; j += DN_NB) {
    const int nb = panel_width(n, j);
    dense_lq_panel_f64<<<1, LQ_PANEL_THREADS, 0, st>>>(A, m, lda, j, nb, tau);
    if (j + nb < n)  // rows below the panel: the panel is a full one
      launch_block(A, lda, j + DN_NB, n - j - DN_NB, A, lda, n, m, j, nb, tau, 0, ws, st);
  }
  return check_launch("fedagg_dense_gelqf_f64");
}

int launch_orglq(const double* A, dn_u64 n, dn_u64 m, dn_u64 lda, const double* tau, double* Q, dn_u64 ldq, double* ws,
                 hipStream_t st) {
  dense_lq_eye_f64<<<dim3(blocks_for(m), (unsigned)(n < 4096 ? n : 4096)), DN_BLOCK, 0, st>>>(Q, n, m, ldq);
  for (dn_u64 j = (n - 1) / DN_NB * DN_NB;; j -= DN_NB) {
    const int nb = panel_width(n, j);
    launch_block(Q, ldq, j, n - j, A, lda, n, m, j, nb, tau, 1, ws, st);
    if (j == 0) break;
  }
  return check_launch("fedagg_dense_orglq_f64");
}

// The argument checks of both entry points (n >= 1 here), before any HIP call.
int check_lq(const void* d_A, dn_u64 n, dn_u64 m, dn_u64 lda, const void* d_tau, const void* d_ws) {
  if (int rc = check_ptr(d_A, "d_A")) return rc;
  if (int rc = check_dim("n", n)) return rc;
  if (int rc = check_dim("m", m)) return rc;
  if (n > m) return fail(FEDAGG_DENSE_EINVAL, "n = %lld is larger than m (the LQ takes n <= m)", (long long)n);
  if (int rc = check_ld("lda", lda, "m", m, n)) return rc;
  if (int rc = check_ptr(d_tau, "d_tau")) return rc;
  if (!d_ws) return fail(FEDAGG_DENSE_EINVAL, "d_ws is NULL (fedagg_dense_lq_ws_bytes(n, m) > 0)");
  return FEDAGG_DENSE_OK;
}

}  // namespace

extern "C" {

int fedagg_dense_lq_blocking(int* panel, int* tile_m, int* tile_n, int* k_chunk) {
  if (!panel || !tile_m || !tile_n || !k_chunk)
    return fail(FEDAGG_DENSE_EINVAL, "fedagg_dense_lq_blocking: NULL output pointer");
  *panel = DN_NB;
  *tile_m = DN_TM;
  *tile_n = DN_TN;
  *k_chunk = LQ_KC;
  return FEDAGG_DENSE_OK;
}

uint64_t fedagg_dense_lq_ws_bytes(uint64_t n, uint64_t m) {
  if (n == 0 || n > m || m > FEDAGG_DENSE_MAX_N) return 0;  // (nothing to factor, or a refused call)
  return ws_doubles(n, m) * 8;
}

int fedagg_dense_gelqf_f64(double* d_A, uint64_t n, uint64_t m, uint64_t lda, double* d_tau, void* d_ws, void* stream) {
  if (n == 0) return FEDAGG_DENSE_OK;
  if (int rc = check_lq(d_A, n, m, lda, d_tau, d_ws)) return rc;
  return launch_gelqf(d_A, n, m, lda, d_tau, (double*)d_ws, (hipStream_t)stream);
}

int fedagg_dense_orglq_f64(const double* d_A, uint64_t n, uint64_t m, uint64_t lda, const double* d_tau, double* d_Q,
                           uint64_t ldq, void* d_ws, void* stream) {
  if (n == 0) return FEDAGG_DENSE_OK;
  if (int rc = check_ptr(d_Q, "d_Q")) return rc;
  if (int rc = check_lq(d_A, n, m, lda, d_tau, d_ws)) return rc;
  if (int rc = check_ld("ldq", ldq, "m", m, n)) return rc;
  return launch_orglq(d_A, n, m, lda, d_tau, d_Q, ldq, (double*)d_ws, (hipStream_t)stream);
}

}  // extern "C"
