// mx.hip -- libfedagg_mx.so (include/fedagg_mx.h): FedAvg over OCP MXFP8 client rows (1-byte
// e4m3fn codes, one e8m0 scale byte per 32 elements) and the quantiser that produces such rows.
//
// The reduction is a streaming kernel like fedavg_kernel of fedagg.hip: a lane's 16-B non-temporal
// load is 16 codes of one client (half a scale block, so one scale byte per load and two lanes
// share it), MX_U clients are loaded ahead of the in-order add chain, and the 16 fp32 results of a
// lane (64 B) are transposed through LDS so that every store instruction of a wave writes one
// contiguous 1 KiB run.
//
// Arithmetic per element and client, three roundings that stay three:
//   x = fl32(v * 2^(s-127))     the decode: exact, or overflow to +-inf
//   p = fl32(x * w_k)           fed_avg.py:221
//   acc = fl32(acc + p)         fed_avg.py:222, client order
// The file is compiled with -ffp-contract=off and every kernel body and helper carries
// `#pragma clang fp contract(off)`.  fp32 denormals are kept (the default of the target): a decoded
// element may be as small as 2^-136.
//
// Two decoders, held to each other and to wire.py by the exhaustive test:
//   - the vector walk: gfx950's v_cvt_pk_f32_fp8 (OCP e4m3fn -> fp32, exact, NaN codes to NaN; every
//     result is a normal fp32) and ONE multiply by the scale constructed from s (2^-127 as the
//     subnormal it is, NaN for s == 255);
//   - plain C++ (the tail elements and the numel == 1 kernel): integer field moves and two
//     multiplies by powers of two, the first of them exact by construction.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "fedagg_mx.h"
#include "pairwise_sum.h"

#define MX_THREADS 256  // threads per workgroup
#define MX_VEC 16       // elements per lane and load: 16 B of codes
#define MX_VPT 1        // vectors per lane and workgroup step (2 with MX_U 4 needs 287 registers, 1 needs 152)
#define MX_U 4          // clients per load group (k_group)
#define MX_TILE (MX_THREADS * MX_VEC * MX_VPT)  // elements per workgroup step (tile_elems)
#define MX_PW_IDX 64    // numel == 1 elements per launch of the pairwise kernel
#define MX_GRID_CAP (1u << 18)

namespace {

using fedagg_internal::pw_leaf;

thread_local char g_error[256] = "";

int fail(int code, const char* fmt, long long v = 0) {
  snprintf(g_error, sizeof(g_error), fmt, v);
  return code;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) return FEDAGG_OK;
  snprintf(g_error, sizeof(g_error), "%s: %s", what, hipGetErrorString(e));
  return FEDAGG_EHIP;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct MxArgs {
  const uint8_t* c[FEDAGG_MX_KCHUNK];  // code rows
  const uint8_t* s[FEDAGG_MX_KCHUNK];  // scale rows
  float w[FEDAGG_MX_KCHUNK];
};

struct MxIdx {
  uint64_t idx[MX_PW_IDX];
  int n;
};

constexpr uint32_t QNAN = 0x7FC00000u;

// 2^(s-127) as the fp32 it is: s == 0 is the subnormal 2^-127; s == 255 poisons the block.
__device__ __forceinline__ float scale_of(uint32_t s) {
  uint32_t b = s << 23;
  if (s == 0) b = 0x00400000u;  // 2^22 * 2^-149
  if (s == 255) b = QNAN;
  return __uint_as_float(b);
}

// Plain C++ decode: the magnitude is q * 2^p with q < 16, p in [-136, 132].  2^p is split into a
// small factor (q * 2^pb is exact) and one in the normal range, so the single rounding is that of
// the last multiply: exact where q * 2^p is an fp32 value (subnormals included), +-inf above.
__device__ __forceinline__ float decode_elem(uint32_t c, uint32_t s) {
#pragma clang fp contract(off)
  if ((c & 0x7Fu) == 0x7Fu || s == 255u) return __uint_as_float(QNAN);
  const int E = (int)((c >> 3) & 15u), m = (int)(c & 7u);
  const int q = E ? 8 + m : m;
  const int p = (E ? E - 10 : -9) + (int)s - 127;
  const int pa = p < -126 ? -126 : (p > 127 ? 127 : p);
  const int pb = p - pa;  // in [-10, 5]
  const float small = (float)q * __uint_as_float((uint32_t)(pb + 127) << 23);
  const float v = small * __uint_as_float((uint32_t)(pa + 127) << 23);
  return (c & 0x80u) ? -v : v;
}

// 16 codes (one 16-B load) to their 16 fp32 values under the scale f.
__device__ __forceinline__ void decode_vec(const u32x4 raw, const float f, float (&x)[MX_VEC]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[d], false);  // bytes 0, 1
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[d], true);   // bytes 2, 3
    x[4 * d + 0] = lo[0] * f;
    x[4 * d + 1] = lo[1] * f;
    x[4 * d + 2] = hi[0] * f;
    x[4 * d + 3] = hi[1] * f;
  }
}

template <int N>
__device__ __forceinline__ void load_group(const MxArgs& a, const int k, const uint64_t (&v)[N], u32x4 (&raw)[N][MX_U],
                                           uint32_t (&sc)[N][MX_U]) {
#pragma unroll
  for (int u = 0; u < MX_U; ++u) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
      raw[n][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.c[k + u]) + v[n]);
      sc[n][u] = a.s[k + u][v[n] >> 1];  // 16 elements are half a block
    }
  }
}

template <int N>
__device__ __forceinline__ void accumulate(const u32x4 (&raw)[N][MX_U], const uint32_t (&sc)[N][MX_U], const float* w,
                                           float (&acc)[N][MX_VEC]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int u = 0; u < MX_U; ++u) {
    const float wu = w[u];
#pragma unroll
    for (int n = 0; n < N; ++n) {
      float x[MX_VEC];
      decode_vec(raw[n][u], scale_of(sc[n][u]), x);
#pragma unroll
      for (int j = 0; j < MX_VEC; ++j) {
        const float p = x[j] * wu;   // fl(x_k * w_k), after the decode's own rounding
        acc[n][j] = acc[n][j] + p;   // fl(acc + p), client order
      }
    }
  }
}

// acc[n][:] = the K clients in order over the N vectors v[n]; groups of MX_U clients are loaded one
// group ahead of the add chain (two register buffers), the last K % MX_U clients one by one.
template <int N>
__device__ __forceinline__ void reduce_vectors(const MxArgs& a, const int K, const int first, const uint64_t (&v)[N],
                                               float (&acc)[N][MX_VEC], const float* out) {
#pragma clang fp contract(off)
#pragma unroll
  for (int n = 0; n < N; ++n) {
    if (first) {
#pragma unroll
      for (int j = 0; j < MX_VEC; ++j) acc[n][j] = 0.0f;  // NumPy seeds add.reduce with +0.0
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const u32x4 r = reinterpret_cast<const u32x4*>(out + v[n] * MX_VEC)[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[n][4 * q + j] = __uint_as_float(r[j]);
      }
    }
  }
  int k = 0;
  if (K >= MX_U) {
    u32x4 ra[N][MX_U], rb[N][MX_U];
    uint32_t sa[N][MX_U], sb[N][MX_U];
    load_group<N>(a, 0, v, ra, sa);
    for (;;) {
      const bool mb = k + 2 * MX_U <= K;
      if (mb) load_group<N>(a, k + MX_U, v, rb, sb);
      accumulate<N>(ra, sa, a.w + k, acc);
      k += MX_U;
      if (!mb) break;
      const bool ma = k + 2 * MX_U <= K;
      if (ma) load_group<N>(a, k + MX_U, v, ra, sa);
      accumulate<N>(rb, sb, a.w + k, acc);
      k += MX_U;
      if (!ma) break;
    }
  }
  for (; k < K; ++k) {
    const float w = a.w[k];
#pragma unroll
    for (int n = 0; n < N; ++n) {
      float x[MX_VEC];
      decode_vec(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.c[k]) + v[n]),
                 scale_of(a.s[k][v[n] >> 1]), x);
#pragma unroll
      for (int j = 0; j < MX_VEC; ++j) {
        const float p = x[j] * w;
        acc[n][j] = acc[n][j] + p;
      }
    }
  }
}

__device__ __forceinline__ void store_direct(float* out, const uint64_t v, const float (&acc)[MX_VEC]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    u32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = __float_as_uint(acc[4 * q + j]);
    __builtin_nontemporal_store(r, reinterpret_cast<u32x4*>(out + v * MX_VEC) + q);
  }
}

// A wave's 64 lanes each own 64 contiguous output bytes of one 4 KiB run.  Stored directly, every
// store instruction would write 16 B per lane at a 64-B stride.  Through 4 KiB of LDS per wave they
// become four fully coalesced 1 KiB stores.  Piece q of lane l (16-B piece j = 4 l + q of the run)
// sits at slot 4 l + ((q + l) & 3): the rotation spreads a store instruction's lanes over the LDS
// banks.  All 64 lanes must be active (the caller checks wave-uniformly).
__device__ __forceinline__ void store_coalesced(float* wave_dst, const float (&acc)[MX_VEC], u32x4* lds_wave) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    u32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = __float_as_uint(acc[4 * q + j]);
    lds_wave[4 * lane + ((q + lane) & 3)] = r;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = q * 64 + lane;  // the 16-B piece this lane stores
    const int l = j >> 2;
    const u32x4 r = lds_wave[4 * l + (((j & 3) + l) & 3)];
    __builtin_nontemporal_store(r, reinterpret_cast<u32x4*>(wave_dst) + j);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // WAR before the buffer is reused
  __builtin_amdgcn_wave_barrier();
}

// nvec: whole 16-element vectors taken by the vector walk (M / 16, or 0 when d_out is not 16-B
// aligned); elements from nvec * 16 on go one by one.
__global__ void __launch_bounds__(MX_THREADS)
    mx_fedavg_kernel(const MxArgs a, const int K, const int first, const uint64_t nvec, const uint64_t M,
                     float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ u32x4 stage[MX_THREADS / 64][256];
  u32x4* lds_wave = stage[threadIdx.x / 64];
  constexpr uint64_t tile = (uint64_t)MX_VPT * MX_THREADS;  // vectors per workgroup step
  for (uint64_t t = blockIdx.x; t * tile < nvec; t += gridDim.x) {
    const uint64_t base = t * tile + threadIdx.x;
    const uint64_t wave_base = base - (threadIdx.x & 63);
    if (base + (MX_VPT - 1) * MX_THREADS < nvec) {
      // wave-uniform: every lane of this wave has all MX_VPT vectors in range
      const bool wave_full = wave_base + 63 + (MX_VPT - 1) * MX_THREADS < nvec;
      uint64_t v[MX_VPT];
#pragma unroll
      for (int n = 0; n < MX_VPT; ++n) v[n] = base + (uint64_t)n * MX_THREADS;
      float acc[MX_VPT][MX_VEC];
      reduce_vectors<MX_VPT>(a, K, first, v, acc, out);
#pragma unroll
      for (int n = 0; n < MX_VPT; ++n) {
        if (wave_full) store_coalesced(out + (wave_base + (uint64_t)n * MX_THREADS) * MX_VEC, acc[n], lds_wave);
        else store_direct(out, v[n], acc[n]);
      }
    } else {
      for (uint64_t v0 = base; v0 < nvec; v0 += MX_THREADS) {
        const uint64_t v[1] = {v0};
        float acc[1][MX_VEC];
        reduce_vectors<1>(a, K, first, v, acc, out);
        store_direct(out, v0, acc[0]);
      }
    }
  }
  // the last M % 16 elements (everything when d_out is not 16-B aligned): plain C++
  const uint64_t stride = (uint64_t)gridDim.x * MX_THREADS;
  for (uint64_t i = nvec * MX_VEC + (uint64_t)blockIdx.x * MX_THREADS + threadIdx.x; i < M; i += stride) {
    float acc = first ? 0.0f : out[i];
    for (int k = 0; k < K; ++k) {
      const float x = decode_elem(a.c[k][i], a.s[k][i >> 5]);
      const float p = x * a.w[k];
      acc = acc + p;
    }
    out[i] = acc;
  }
}

// numel == 1 elements: one leaf (n <= 128 terms) of NumPy's pairwise tree over the products of the
// n clients in `a`, one lane per element.  add: the running node value in out[i] is the other
// operand of this node's sum; fin: this is the tree's root, and NumPy's reduction adds it to +0.0.
__global__ void __launch_bounds__(MX_PW_IDX)
    mx_pairwise_kernel(const MxArgs a, const MxIdx ix, const int n, const int add, const int fin,
                       float* __restrict__ out) {
#pragma clang fp contract(off)
  if ((int)threadIdx.x >= ix.n) return;
  const uint64_t i = ix.idx[threadIdx.x];
  auto get = [&](int64_t k) -> float {
    const float x = decode_elem(a.c[k][i], a.s[k][i >> 5]);
    return x * a.w[k];
  };
  float r = pw_leaf<float>(get, 0, n);
  if (add) r = out[i] + r;
  if (fin) r = 0.0f + r;
  out[i] = r;
}

// ------------------------------------------------------------------------------------
// Quantiser: one element per lane, the 32 lanes of a half-wave are one scale block.
// ------------------------------------------------------------------------------------
// fp32 bits of a finite |y| to the e4m3fn magnitude code: nearest even, 448 and above to 0x7E.
__device__ __forceinline__ uint32_t e4m3_of(const uint32_t a) {
#pragma clang fp contract(off)
  if (a >= 0x43E00000u) return 0x7Eu;  // 448
  if (a < 0x3C800000u) {               // below 2^-6 the values are the multiples of 2^-9:
    const float f = __uint_as_float(a) + 16384.0f;  // 2^14 has ulp 2^-9, the add rounds to it
    return __float_as_uint(f) - 0x46800000u;
  }
  return (a + 0x7FFFFu + ((a >> 20) & 1u) - 0x3C000000u) >> 20;
}

template <int KIND>
__global__ void __launch_bounds__(MX_THREADS)
    mx_quantize_kernel(const void* __restrict__ x_, const uint64_t M, uint8_t* __restrict__ codes,
                       uint8_t* __restrict__ scales) {
#pragma clang fp contract(off)
  const uint64_t padded = (M + 31) & ~(uint64_t)31;  // every lane of a block walks the same steps
  const uint64_t stride = (uint64_t)gridDim.x * MX_THREADS;
  for (uint64_t i = (uint64_t)blockIdx.x * MX_THREADS + threadIdx.x; i < padded; i += stride) {
    uint32_t u = 0;  // lanes past M hold +0: no effect on the maximum
    if (i < M) {
      if constexpr (KIND == FEDAGG_BF16) u = (uint32_t)static_cast<const uint16_t*>(x_)[i] << 16;
      else u = static_cast<const uint32_t*>(x_)[i];
    }
    const uint32_t mag = u & 0x7FFFFFFFu;
    // max |x| over the block's 32 lanes as the maximum of the magnitudes' bit patterns (NaN and Inf
    // sort above every finite value)
    uint32_t a = mag;
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)a, d, 32);
      a = o > a ? o : a;
    }
    uint32_t s, code;
    if (a >= 0x7F800000u) {
      s = 255u;
      code = 0u;
    } else if (a == 0u) {
      s = 127u;
      code = (u >> 24) & 0x80u;
    } else {
      int fl;         // floor(log2(amax))
      uint32_t mant;  // amax's 24 significant bits, the leading one at bit 23
      if (a < 0x00800000u) {
        const int lz = __builtin_clz(a);
        fl = 31 - lz - 149;
        mant = a << (lz - 8);
      } else {
        fl = (int)(a >> 23) - 127;
        mant = (a & 0x007FFFFFu) | 0x00800000u;
      }
      int e = fl - 8;
      if (mant > 0x00E80000u) e += 1;  // amax * 2^-e > 464 = 1.8125 * 2^8
      e = e < -127 ? -127 : (e > 127 ? 127 : e);
      s = (uint32_t)(e + 127);
      const uint32_t f = (uint32_t)(127 - e);                               // exponent field of 2^-e
      const float inv = __uint_as_float(f ? f << 23 : 0x00400000u);        // 2^-127 is a subnormal
      const float y = __uint_as_float(u) * inv;
      const uint32_t yu = __float_as_uint(y);
      code = e4m3_of(yu & 0x7FFFFFFFu) | ((yu >> 24) & 0x80u);
    }
    if (i < M) {
      codes[i] = (uint8_t)code;
      if ((i & 31) == 0) scales[i >> 5] = (uint8_t)s;
    }
  }
}

unsigned grid_for(uint64_t work_items, uint64_t per_block) {
  uint64_t g = (work_items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return (unsigned)(g > MX_GRID_CAP ? MX_GRID_CAP : g);
}

void fill_args(MxArgs& a, const uint8_t* const* codes, const uint8_t* const* scales, const float* w, int k0, int n) {
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < n; ++k) {
    a.c[k] = codes[k0 + k];
    a.s[k] = scales[k0 + k];
    a.w[k] = w[k0 + k];
  }
}

}  // namespace

extern "C" {

int fedagg_mx_abi_version(void) { return FEDAGG_MX_ABI_VERSION; }
const char* fedagg_mx_last_error(void) { return g_error; }

int fedagg_mx_blocking(int* tile_elems, int* k_group) {
  if (tile_elems) *tile_elems = MX_TILE;
  if (k_group) *k_group = MX_U;
  return FEDAGG_OK;
}

int fedagg_mx_fedavg_e4m3(const uint8_t* const* d_codes, const uint8_t* const* d_scales, const float* h_w, int K,
                          uint64_t M, const uint64_t* h_idx, int P, float* d_out, void* stream) {
  if (K <= 0) return fail(FEDAGG_EINVAL, "mx fedavg: K must be positive (K=%lld)", K);
  if (!d_codes) return fail(FEDAGG_EINVAL, "mx fedavg: d_codes is NULL");
  if (!d_scales) return fail(FEDAGG_EINVAL, "mx fedavg: d_scales is NULL");
  if (!h_w) return fail(FEDAGG_EINVAL, "mx fedavg: h_w is NULL");
  if (P < 0) return fail(FEDAGG_EINVAL, "mx fedavg: P is negative (P=%lld)", P);
  if (P > 0 && !h_idx) return fail(FEDAGG_EINVAL, "mx fedavg: h_idx is NULL with P > 0");
  if (M == 0) return FEDAGG_OK;
  if (M > (1ull << 44)) return fail(FEDAGG_EINVAL, "mx fedavg: M is too large");
  for (int k = 0; k < K; ++k) {
    if (!d_codes[k]) return fail(FEDAGG_EINVAL, "mx fedavg: code row %lld is NULL", k);
    if (reinterpret_cast<uintptr_t>(d_codes[k]) & 15u)
      return fail(FEDAGG_EINVAL, "mx fedavg: code row %lld is not 16-B aligned", k);
    if (!d_scales[k]) return fail(FEDAGG_EINVAL, "mx fedavg: scale row %lld is NULL", k);
  }
  if (!d_out) return fail(FEDAGG_EINVAL, "mx fedavg: d_out is NULL");
  if (reinterpret_cast<uintptr_t>(d_out) & 3u) return fail(FEDAGG_EINVAL, "mx fedavg: d_out is not 4-B aligned");
  for (int p = 0; p < P; ++p)
    if (h_idx[p] >= M) return fail(FEDAGG_EINVAL, "mx fedavg: numel == 1 index %lld is out of range", p);
  if (P > 0 && K > FEDAGG_MX_MAX_PAIRWISE_K)
    return fail(FEDAGG_EINVAL, "mx fedavg: numel == 1 elements are served up to FEDAGG_MX_MAX_PAIRWISE_K clients (K=%lld)", K);

  const uint64_t nvec = (reinterpret_cast<uintptr_t>(d_out) & 15u) ? 0 : M / MX_VEC;
  const unsigned grid = grid_for(M, MX_TILE);
  MxArgs a;
  for (int k0 = 0; k0 < K; k0 += FEDAGG_MX_KCHUNK) {
    const int n = K - k0 < FEDAGG_MX_KCHUNK ? K - k0 : FEDAGG_MX_KCHUNK;
    fill_args(a, d_codes, d_scales, h_w, k0, n);
    hipLaunchKernelGGL(mx_fedavg_kernel, dim3(grid), dim3(MX_THREADS), 0, (hipStream_t)stream, a, n, k0 == 0 ? 1 : 0,
                       nvec, M, d_out);
    const int rc = check_launch("mx fedavg kernel");
    if (rc) return rc;
  }
  if (P == 0) return FEDAGG_OK;

  // NumPy's pairwise tree over the K products (loops_utils.h.src: a leaf up to 128 terms, else
  // split at n / 2 rounded down to a multiple of 8).  Up to 256 terms every inner node has a leaf
  // child, so a node's value waits in d_out[i] for that leaf and nothing else is pending (IEEE
  // addition commutes, so which operand waits does not matter).
  struct Step { int lo, n, add, fin; } steps[3];
  int nsteps = 0;
  if (K <= 128) {
    steps[nsteps++] = {0, K, 0, 1};
  } else {
    int n2 = K / 2;
    n2 -= n2 % 8;
    const int right = K - n2;
    if (right <= 128) {
      steps[nsteps++] = {0, n2, 0, 0};
      steps[nsteps++] = {n2, right, 1, 1};
    } else {  // the right half is two leaves: it goes first, the left leaf joins last
      int r2 = right / 2;
      r2 -= r2 % 8;
      steps[nsteps++] = {n2, r2, 0, 0};
      steps[nsteps++] = {n2 + r2, right - r2, 1, 0};
      steps[nsteps++] = {0, n2, 1, 1};
    }
  }
  for (int p0 = 0; p0 < P; p0 += MX_PW_IDX) {
    MxIdx ix;
    memset(&ix, 0, sizeof(ix));
    ix.n = P - p0 < MX_PW_IDX ? P - p0 : MX_PW_IDX;
    for (int p = 0; p < ix.n; ++p) ix.idx[p] = h_idx[p0 + p];
    for (int st = 0; st < nsteps; ++st) {
      fill_args(a, d_codes, d_scales, h_w, steps[st].lo, steps[st].n);
      hipLaunchKernelGGL(mx_pairwise_kernel, dim3(1), dim3(MX_PW_IDX), 0, (hipStream_t)stream, a, ix, steps[st].n,
                         steps[st].add, steps[st].fin, d_out);
      const int rc = check_launch("mx pairwise kernel");
      if (rc) return rc;
    }
  }
  return FEDAGG_OK;
}

int fedagg_mx_quantize(const void* d_x, int kind, uint64_t M, uint8_t* d_codes, uint8_t* d_scales, void* stream) {
  if (kind != FEDAGG_F32 && kind != FEDAGG_BF16)
    return fail(FEDAGG_EINVAL, "mx quantize: kind %lld is not FEDAGG_F32 / FEDAGG_BF16", kind);
  if (M == 0) return FEDAGG_OK;
  if (M > (1ull << 44)) return fail(FEDAGG_EINVAL, "mx quantize: M is too large");
  if (!d_x) return fail(FEDAGG_EINVAL, "mx quantize: d_x is NULL");
  if (reinterpret_cast<uintptr_t>(d_x) & (kind == FEDAGG_F32 ? 3u : 1u))
    return fail(FEDAGG_EINVAL, "mx quantize: d_x is not aligned to its element size");
  if (!d_codes) return fail(FEDAGG_EINVAL, "mx quantize: d_codes is NULL");
  if (!d_scales) return fail(FEDAGG_EINVAL, "mx quantize: d_scales is NULL");
  const unsigned grid = grid_for(M, MX_THREADS);
  if (kind == FEDAGG_F32)
    hipLaunchKernelGGL(mx_quantize_kernel<FEDAGG_F32>, dim3(grid), dim3(MX_THREADS), 0, (hipStream_t)stream, d_x, M,
                       d_codes, d_scales);
  else
    hipLaunchKernelGGL(mx_quantize_kernel<FEDAGG_BF16>, dim3(grid), dim3(MX_THREADS), 0, (hipStream_t)stream, d_x, M,
                       d_codes, d_scales);
  return check_launch("mx quantize kernel");
}

}  // extern "C"
