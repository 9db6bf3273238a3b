// scaffold16.hip -- fedagg_scaffold_bucket: ONE Scaffold bucket per call, rows of any float kind.
//
// Scaffold's two sums (scaffold.py:262-263 the control variate, :293 the delta) are independent,
// and the reference multiplies every array by a float64 weight (a strong scalar under NEP 50), so
// each product and sum is fp64 on the exact upcast of the input whatever the input's dtype.  A
// 16-bit model's buckets are therefore read as they are -- 2 bytes per element and client -- and
// widened in registers: bf16 -> fp32 is a 16-bit shift, fp16 -> fp32 -> fp64 are exact converts.
//
//   phase 0:  out[i] = lr * (+0.0 + sum_seq_k fl64(w_k * (double)x_k[i]))
//   phase 1:  out[i] =       (+0.0 + sum_seq_k fl64(w_k * (double)x_k[i])) + (double)c[i]
//
// One walk serves the four row kinds (a lane loads 16 B = L elements, keeps L fp64 accumulators
// per vector and stores 8 * L bytes); fp32 / fp64 rows give the bytes of fedagg_scaffold_f32 /
// _f64 (same per-element order, no contraction).  The server control variate c is read once per
// element in the epilogue, in its own kind.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "fedagg_internal.h"
#include "pairwise_sum.h"

using fedagg_internal::check_launch;
using fedagg_internal::fail;
using fedagg_internal::pw_leaf;
using fedagg_internal::pw_sum;

namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int KC = FEDAGG_KCHUNK_SCAFFOLD;

// Element kinds: storage type T, exact widening to fp64.
struct KF16 {
  using T = uint16_t;
  __device__ static double widen(T b) {
    _Float16 h;
    __builtin_memcpy(&h, &b, 2);
    return (double)(float)h;
  }
};
struct KBF16 {
  using T = uint16_t;
  __device__ static double widen(T b) { return (double)__uint_as_float(((uint32_t)b) << 16); }
};
struct KF32 {
  using T = float;
  __device__ static double widen(T v) { return (double)v; }
};
struct KF64 {
  using T = double;
  __device__ static double widen(T v) { return v; }
};

// The 16 / sizeof(T) elements of one 16-byte vector, widened.
template <typename E>
__device__ __forceinline__ void unpack(u32x4 r, double* o) {
  if constexpr (sizeof(typename E::T) == 2) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[2 * j] = E::widen((uint16_t)(r[j] & 0xFFFFu));
      o[2 * j + 1] = E::widen((uint16_t)(r[j] >> 16));
    }
  } else if constexpr (sizeof(typename E::T) == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (double)__uint_as_float(r[j]);
  } else {
    o[0] = __hiloint2double((int)r[1], (int)r[0]);
    o[1] = __hiloint2double((int)r[3], (int)r[2]);
  }
}

__device__ __forceinline__ u32x4 ld16_nt(const void* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}
__device__ __forceinline__ void st16_nt(void* p, u32x4 v) {
  __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
}

struct BkArgs {
  const void* x[KC];
  double w[KC];
};
struct PwArgs {  // numel == 1 element indices patched inside the bucket launch
  uint64_t idx[FEDAGG_FUSED_PAIRWISE];
  int n;
};
struct IdxArgs {
  uint64_t idx[FEDAGG_MAX_PAIRWISE];
};

template <typename E>
__device__ __forceinline__ double row_at(const BkArgs& a, int k, uint64_t i) {
  return E::widen(static_cast<const typename E::T*>(a.x[k])[i]);
}

__device__ __forceinline__ double c_at(const void* c, int ck, uint64_t i) {
  switch (ck) {
    case FEDAGG_F16: return KF16::widen(static_cast<const uint16_t*>(c)[i]);
    case FEDAGG_BF16: return KBF16::widen(static_cast<const uint16_t*>(c)[i]);
    case FEDAGG_F32: return (double)static_cast<const float*>(c)[i];
    default: return static_cast<const double*>(c)[i];
  }
}

// c[e0 .. e0 + L) widened, e0 a multiple of L and c 16-B aligned: whole 16-byte loads where L
// elements of the kind fill at least one.
template <typename C, int L>
__device__ __forceinline__ void c_vec_kind(const void* c, uint64_t e0, double* xc) {
  using T = typename C::T;
  if constexpr (L * sizeof(T) >= 16) {
    constexpr int PER = 16 / sizeof(T);
#pragma unroll
    for (int s = 0; s < L / PER; ++s) unpack<C>(ld16_nt(static_cast<const T*>(c) + e0 + s * PER), xc + s * PER);
  } else {
#pragma unroll
    for (int j = 0; j < L; ++j) xc[j] = C::widen(static_cast<const T*>(c)[e0 + j]);
  }
}
template <int L>
__device__ __forceinline__ void c_vec(const void* c, int ck, uint64_t e0, double* xc) {
  switch (ck) {  // wave-uniform
    case FEDAGG_F16: return c_vec_kind<KF16, L>(c, e0, xc);
    case FEDAGG_BF16: return c_vec_kind<KBF16, L>(c, e0, xc);
    case FEDAGG_F32: return c_vec_kind<KF32, L>(c, e0, xc);
    default: return c_vec_kind<KF64, L>(c, e0, xc);
  }
}

// The numel == 1 element e inside the launch (K <= KC, so one leaf of the pairwise tree):
// phase 0 lr * (0 + pw_K(w * x)), phase 1 0 + pw_{K+1}(w * x, c).
template <typename E>
__device__ __forceinline__ double pairwise_elem(const BkArgs& a, int K, int phase, const void* c, int ck, double lr,
                                                uint64_t e) {
#pragma clang fp contract(off)
  if (phase == 0) {
    auto g = [&](int64_t k) -> double { return a.w[k] * row_at<E>(a, (int)k, e); };
    const double s = 0.0 + pw_leaf<double>(g, 0, K);
    return lr * s;
  }
  auto g = [&](int64_t k) -> double { return k < K ? a.w[k] * row_at<E>(a, (int)k, e) : c_at(c, ck, e); };
  return 0.0 + pw_leaf<double>(g, 0, K + 1);
}

template <typename E, int N, int SU>
__device__ __forceinline__ void load_group(const BkArgs& a, const int k, const uint64_t* v, u32x4 (&r)[N][SU]) {
  constexpr int L = 16 / sizeof(typename E::T);
#pragma unroll
  for (int u = 0; u < SU; ++u)
#pragma unroll
    for (int n = 0; n < N; ++n) r[n][u] = ld16_nt(static_cast<const typename E::T*>(a.x[k + u]) + v[n] * L);
}

// fp64 products and in-order adds of one loaded group (w_k * x_k summed in list order).
template <typename E, int N, int SU>
__device__ __forceinline__ void add_group(const BkArgs& a, const int k, const u32x4 (&r)[N][SU],
                                          double (&acc)[N][16 / sizeof(typename E::T)]) {
#pragma clang fp contract(off)
  constexpr int L = 16 / sizeof(typename E::T);
#pragma unroll
  for (int u = 0; u < SU; ++u) {
    const double w = a.w[k + u];
#pragma unroll
    for (int n = 0; n < N; ++n) {
      double x[L];
      unpack<E>(r[n][u], x);
#pragma unroll
      for (int j = 0; j < L; ++j) {
        const double p = w * x[j];
        acc[n][j] = acc[n][j] + p;
      }
    }
  }
}

// A wave's 64 lanes each own 8 * L contiguous output bytes of one run (NS = L / 2 16-byte
// pieces per lane).  Stored directly, every store instruction would write 16 B per lane at an
// 8 * L-byte stride; transposing through LDS turns them into NS fully coalesced 1-KiB store
// instructions.  Requires all 64 lanes active (callers check wave-uniformly).
template <int NS>
__device__ __forceinline__ void store_wave(double* wave_dst, const u32x4 (&r)[NS], u32x4* lds_wave) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int s = 0; s < NS; ++s) lds_wave[NS * lane + s] = r[s];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int s = 0; s < NS; ++s) st16_nt(reinterpret_cast<u32x4*>(wave_dst) + 64 * s + lane, lds_wave[64 * s + lane]);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // WAR before the buffer is reused
  __builtin_amdgcn_wave_barrier();
}

// N 16-byte vectors of the bucket: the in-order fp64 sum over this chunk's K clients, then (last
// chunk) * lr or + c, the fused numel == 1 patch and the fp64 stores.  PIPE: the next client
// group's loads are issued before this group's products and adds.
template <typename E, int N, int SU, bool PIPE>
__device__ __forceinline__ void bucket_vectors(const BkArgs& a, const PwArgs& pw, const int K, const int first,
                                               const int last, const int phase, const void* __restrict__ c,
                                               const int ck, const double lr, const uint64_t* v,
                                               double* __restrict__ out, bool wave_full, u32x4* lds_wave) {
#pragma clang fp contract(off)
  constexpr int L = 16 / sizeof(typename E::T);
  double acc[N][L];
#pragma unroll
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int j = 0; j < L; ++j) acc[n][j] = first ? 0.0 : out[v[n] * L + j];
  int k = 0;
  if constexpr (PIPE) {
    if (K >= SU) {
      u32x4 ra[N][SU], rb[N][SU];
      load_group<E, N, SU>(a, 0, v, ra);
      for (;;) {
        const bool mb = k + 2 * SU <= K;
        if (mb) load_group<E, N, SU>(a, k + SU, v, rb);
        add_group<E, N, SU>(a, k, ra, acc);
        k += SU;
        if (!mb) break;
        const bool ma = k + 2 * SU <= K;
        if (ma) load_group<E, N, SU>(a, k + SU, v, ra);
        add_group<E, N, SU>(a, k, rb, acc);
        k += SU;
        if (!ma) break;
      }
    }
  } else {
    for (; k + SU <= K; k += SU) {
      u32x4 r[N][SU];
      load_group<E, N, SU>(a, k, v, r);
      add_group<E, N, SU>(a, k, r, acc);
    }
  }
  for (; k < K; ++k) {  // clients past the last whole group
    u32x4 r[N][1];
    load_group<E, N, 1>(a, k, v, r);
    add_group<E, N, 1>(a, k, r, acc);
  }
  if (last) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
      if (phase == 0) {
#pragma unroll
        for (int j = 0; j < L; ++j) acc[n][j] = lr * acc[n][j];  // scaffold.py:293
      } else {
        double xc[L];
        c_vec<L>(c, ck, v[n] * L, xc);
#pragma unroll
        for (int j = 0; j < L; ++j) acc[n][j] = acc[n][j] + xc[j];  // c last (scaffold.py:262-263)
      }
    }
  }
  for (int p = 0; p < pw.n; ++p) {
    const uint64_t e = pw.idx[p];
    int owner = -1;
#pragma unroll
    for (int n = 0; n < N; ++n)
      if (e / L == v[n]) owner = n;
    if (owner >= 0) {
      const double val = pairwise_elem<E>(a, K, phase, c, ck, lr, e);
      const int j = (int)(e % L);
#pragma unroll
      for (int n = 0; n < N; ++n)
#pragma unroll
        for (int jj = 0; jj < L; ++jj)
          if (n == owner && jj == j) acc[n][jj] = val;
    }
  }
#pragma unroll
  for (int n = 0; n < N; ++n) {
    u32x4 r[L / 2];
#pragma unroll
    for (int s = 0; s < L / 2; ++s) {
      const f64x2 t = {acc[n][2 * s], acc[n][2 * s + 1]};
      r[s] = __builtin_bit_cast(u32x4, t);
    }
    if constexpr (L > 2) {
      if (wave_full) {
        store_wave<L / 2>(out + (v[n] - (threadIdx.x & 63)) * L, r, lds_wave);
        continue;
      }
    }
#pragma unroll
    for (int s = 0; s < L / 2; ++s) st16_nt(reinterpret_cast<u32x4*>(out + v[n] * L) + s, r[s]);
  }
}

// A workgroup step covers VPT * FA_BLOCK contiguous vectors (thread t: vectors t, t + FA_BLOCK,
// ...); workgroups grid-stride over the steps.  nvec = 0 (an operand not 16-B aligned): every
// element takes the scalar loop, which also serves the M % L tail.
template <typename E, int VPT, int SU, bool PIPE>
__global__ void __launch_bounds__(FA_BLOCK)
    scaffold_rows_kernel(const BkArgs a, const PwArgs pw, const int K, const int first, const int last,
                         const int phase, const void* __restrict__ c, const int ck, const double lr,
                         const uint64_t nvec, const uint64_t M, double* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int L = 16 / sizeof(typename E::T);
  constexpr int LDS_PER_WAVE = L > 2 ? 64 * (L / 2) : 1;
  __shared__ u32x4 stage[FA_BLOCK / 64][LDS_PER_WAVE];
  u32x4* lds_wave = stage[threadIdx.x / 64];
  const uint64_t tile = (uint64_t)VPT * FA_BLOCK;
  for (uint64_t t = blockIdx.x; t * tile < nvec; t += gridDim.x) {
    const uint64_t base = t * tile + threadIdx.x;
    const bool wave_full = (base - (threadIdx.x & 63)) + 63 + (VPT - 1) * FA_BLOCK < nvec;
    if (base + (VPT - 1) * FA_BLOCK < nvec) {
      uint64_t v[VPT];
#pragma unroll
      for (int n = 0; n < VPT; ++n) v[n] = base + n * FA_BLOCK;
      bucket_vectors<E, VPT, SU, PIPE>(a, pw, K, first, last, phase, c, ck, lr, v, out, wave_full, lds_wave);
    } else {
      for (uint64_t v0 = base; v0 < nvec; v0 += FA_BLOCK)
        bucket_vectors<E, 1, SU, false>(a, pw, K, first, last, phase, c, ck, lr, &v0, out, false, lds_wave);
    }
  }
  for (uint64_t i = nvec * L + (uint64_t)blockIdx.x * FA_BLOCK + threadIdx.x; i < M;
       i += (uint64_t)gridDim.x * FA_BLOCK) {
    double acc = first ? 0.0 : out[i];
    for (int k = 0; k < K; ++k) {
      const double p = a.w[k] * row_at<E>(a, k, i);
      acc = acc + p;
    }
    if (last) acc = phase == 0 ? lr * acc : acc + c_at(c, ck, i);
    for (int p = 0; p < pw.n; ++p)
      if (pw.idx[p] == i) acc = pairwise_elem<E>(a, K, phase, c, ck, lr, i);
    out[i] = acc;
  }
}

// The separate numel == 1 path (K > KC or P > FEDAGG_FUSED_PAIRWISE).  Stage 1: the products of
// one client chunk into columns kbase.. of ws[P][stride].
template <typename E>
__global__ void __launch_bounds__(FA_BLOCK)
    bucket_gather_kernel(const BkArgs a, const int Kc, const int kbase, const IdxArgs ix, const int P,
                         const int64_t stride, double* __restrict__ ws) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * FA_BLOCK + threadIdx.x;
  if (t >= P * Kc) return;
  const int p = t / Kc, k = t % Kc;
  ws[p * stride + kbase + k] = a.w[k] * row_at<E>(a, k, ix.idx[p]);
}

// Stage 2: NumPy's pairwise tree over the K terms (phase 0, then * lr) or the K + 1 terms
// (phase 1: c is the last term, scaffold.py:262).
__global__ void bucket_tree_kernel(double* __restrict__ ws, const int64_t K, const int phase, const void* c,
                                   const int ck, const IdxArgs ix, const int P, const double lr,
                                   double* __restrict__ out) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  double* row = ws + p * (K + phase);
  if (phase) row[K] = c_at(c, ck, ix.idx[p]);
  auto g = [&](int64_t i) -> double { return row[i]; };
  const double s = 0.0 + pw_sum<double>(g, K + phase);
  out[ix.idx[p]] = phase ? s : lr * s;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The one dispatched shape of each row kind: 16-byte vectors per thread and step, clients per
// load group, software-pipelined groups.
template <typename E>
struct Shape;
// 2-byte rows, 2 x 4 (117 VGPRs, 4 waves/SIMD), measured over 16 x 25M and 64 x 25M
// (profiles/scaffold16_shapes.log): the tiles that keep 4-5 waves per SIMD (1 x 4, 1 x 8, 2 x 2,
// 2 x 4, 2 x 8) sit within 3 % of each other -- 64 x 25M fp16 1.17-1.24 ms, bf16 1.18-1.23 --
// and there fp16 and bf16 cost the same, so the converts are hidden; the wider ones are slower and
// fp16 then falls behind bf16 (4 x 4: 1.42 / 1.28 ms, 4 x 8: 1.92 / 1.25, 8 x 2: 2.04 / 1.37).
// Software-pipelined groups change nothing (2 x 4: 1.18 / 1.21).  Of the plateau 2 x 4 has the
// smallest load group that still keeps two vectors in flight per lane, which matters to
// federations of a handful of clients (fewer than SU clients are walked one at a time).
// Untransposed 64-B-per-lane stores cost 24 % at 16 x 25M (4 x 4: 0.499 against 0.402 ms).
template <>
struct Shape<KF16> {
  static constexpr int VPT = 2, SU = 4;
  static constexpr bool PIPE = false;
};
template <>
struct Shape<KBF16> : Shape<KF16> {};
template <>
struct Shape<KF32> {  // the tile of fedagg_scaffold_f32's one-bucket launches
  static constexpr int VPT = 8, SU = 4;
  static constexpr bool PIPE = false;
};
template <>
struct Shape<KF64> {  // and of fedagg_scaffold_f64's
  static constexpr int VPT = 4, SU = 2;
  static constexpr bool PIPE = true;
};

template <typename E>
int bucket_launch(const void* const* rows, const double* w, int K, uint64_t M, int phase, const void* c, int ck,
                  double lr, const uint64_t* idx, int P, void* ws, double* out, hipStream_t s) {
  using T = typename E::T;
  constexpr int L = 16 / sizeof(T);
  constexpr int VPT = Shape<E>::VPT, SU = Shape<E>::SU;
  constexpr bool PIPE = Shape<E>::PIPE;
  bool vec = aligned16(out) && (phase == 0 || aligned16(c));
  for (int k = 0; k < K; ++k) vec = vec && aligned16(rows[k]);
  const bool fuse = fedagg_internal::fuse_pairwise() && P <= FEDAGG_FUSED_PAIRWISE && K <= KC;
  if (P > 0 && !fuse && !ws)
    return fail(FEDAGG_EINVAL, "scaffold_bucket: workspace needed for %lld pairwise segments", P);
  const uint64_t nvec = vec ? M / L : 0;
  const unsigned grid = fedagg_internal::launch_grid(nvec ? (nvec + VPT - 1) / VPT : M);
  for (int k0 = 0; k0 < K; k0 += KC) {
    const int kc = (K - k0) < KC ? (K - k0) : KC;
    BkArgs a;
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < kc; ++k) {
      a.x[k] = rows[k0 + k];
      a.w[k] = w[k0 + k];
    }
    PwArgs pw;
    memset(&pw, 0, sizeof(pw));
    if (fuse) {
      pw.n = P;
      for (int p = 0; p < P; ++p) pw.idx[p] = idx[p];
    }
    hipLaunchKernelGGL((scaffold_rows_kernel<E, VPT, SU, PIPE>), dim3(grid), dim3(FA_BLOCK), 0, s, a, pw, kc,
                       (int)(k0 == 0), (int)(k0 + kc == K), phase, c, ck, lr, nvec, M, out);
    const int rc = check_launch("scaffold_rows_kernel");
    if (rc) return rc;
  }
  if (P == 0 || fuse) return FEDAGG_OK;
  const int64_t stride = (int64_t)K + phase;
  for (int p0 = 0; p0 < P; p0 += FEDAGG_MAX_PAIRWISE) {
    const int pc = (P - p0) < FEDAGG_MAX_PAIRWISE ? (P - p0) : FEDAGG_MAX_PAIRWISE;
    IdxArgs ix;
    memset(&ix, 0, sizeof(ix));
    for (int p = 0; p < pc; ++p) ix.idx[p] = idx[p0 + p];
    for (int k0 = 0; k0 < K; k0 += KC) {
      const int kc = (K - k0) < KC ? (K - k0) : KC;
      BkArgs a;
      memset(&a, 0, sizeof(a));
      for (int k = 0; k < kc; ++k) {
        a.x[k] = rows[k0 + k];
        a.w[k] = w[k0 + k];
      }
      hipLaunchKernelGGL((bucket_gather_kernel<E>), dim3((unsigned)((pc * kc + FA_BLOCK - 1) / FA_BLOCK)),
                         dim3(FA_BLOCK), 0, s, a, kc, k0, ix, pc, stride, static_cast<double*>(ws));
      const int rc = check_launch("bucket_gather_kernel");
      if (rc) return rc;
    }
    hipLaunchKernelGGL(bucket_tree_kernel, dim3(1), dim3(64), 0, s, static_cast<double*>(ws), (int64_t)K, phase, c,
                       ck, ix, pc, lr, out);
    const int rc = check_launch("bucket_tree_kernel");
    if (rc) return rc;
  }
  return FEDAGG_OK;
}

inline bool float_kind(int kind) {
  return kind == FEDAGG_F16 || kind == FEDAGG_BF16 || kind == FEDAGG_F32 || kind == FEDAGG_F64;
}

}  // namespace

extern "C" {

uint64_t fedagg_scaffold_bucket_tile(int row_kind) {
  switch (row_kind) {
    case FEDAGG_F16:
    case FEDAGG_BF16: return (uint64_t)Shape<KF16>::VPT * FA_BLOCK * 8;
    case FEDAGG_F32: return (uint64_t)Shape<KF32>::VPT * FA_BLOCK * 4;
    case FEDAGG_F64: return (uint64_t)Shape<KF64>::VPT * FA_BLOCK * 2;
    default: return 0;
  }
}

int fedagg_scaffold_bucket(const void* const* d_rows, int row_kind, const double* h_w, int K, uint64_t M, int phase,
                           const void* d_c, int c_kind, double lr, const uint64_t* h_idx, int P, void* d_ws,
                           double* d_out, void* stream) {
  if (K <= 0) return fail(FEDAGG_EINVAL, "scaffold_bucket: K must be > 0 (got %lld)", K);
  if (!d_rows || !h_w || !d_out) return fail(FEDAGG_EINVAL, "scaffold_bucket: NULL argument");
  if (phase != 0 && phase != 1) return fail(FEDAGG_EINVAL, "scaffold_bucket: phase must be 0 or 1 (got %lld)", phase);
  if (!float_kind(row_kind)) return fail(FEDAGG_EINVAL, "scaffold_bucket: unknown row kind %lld", row_kind);
  if (phase == 1) {
    if (!d_c) return fail(FEDAGG_EINVAL, "scaffold_bucket: phase 1 needs the server control variate (NULL d_c)");
    if (!float_kind(c_kind)) return fail(FEDAGG_EINVAL, "scaffold_bucket: unknown c kind %lld", c_kind);
    if ((row_kind == FEDAGG_F32 || row_kind == FEDAGG_F64) && c_kind != row_kind)
      return fail(FEDAGG_EINVAL, "scaffold_bucket: c kind %lld must equal the kind of f32 / f64 rows", c_kind);
  }
  if (P < 0 || (P > 0 && !h_idx)) return fail(FEDAGG_EINVAL, "scaffold_bucket: bad pairwise index list (P=%lld)", P);
  for (int p = 0; p < P; ++p)
    if (h_idx[p] >= M)
      return fail(FEDAGG_EINVAL, "scaffold_bucket: pairwise index %lld out of range", (long long)h_idx[p]);
  for (int k = 0; k < K; ++k)
    if (!d_rows[k]) return fail(FEDAGG_EINVAL, "scaffold_bucket: client pointer %lld is NULL", k);
  if (M == 0) return FEDAGG_OK;
  hipStream_t s = (hipStream_t)stream;
  switch (row_kind) {
    case FEDAGG_F16: return bucket_launch<KF16>(d_rows, h_w, K, M, phase, d_c, c_kind, lr, h_idx, P, d_ws, d_out, s);
    case FEDAGG_BF16: return bucket_launch<KBF16>(d_rows, h_w, K, M, phase, d_c, c_kind, lr, h_idx, P, d_ws, d_out, s);
    case FEDAGG_F32: return bucket_launch<KF32>(d_rows, h_w, K, M, phase, d_c, c_kind, lr, h_idx, P, d_ws, d_out, s);
    default: return bucket_launch<KF64>(d_rows, h_w, K, M, phase, d_c, c_kind, lr, h_idx, P, d_ws, d_out, s);
  }
}

}  // extern "C"
