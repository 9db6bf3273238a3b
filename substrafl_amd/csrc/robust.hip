// robust.hip -- libfedagg_robust.so (include/fedagg_robust.h): the coordinate-wise trimmed mean over
// K client rows, the median as its limit case.
//
// FedAvg streams the clients through one accumulator; a trimmed mean needs all K values of an
// element at once and has to order them.  Here they live in registers.  A lane owns VEC consecutive
// elements and holds, for each of them, one sortable key per client: KP keys, K padded to the next
// power of two in 2 .. 128.  A fully unrolled sorting network (Batcher's odd-even merge sort: 1, 3,
// 9, 25, 63, 191, 543, 1471 exchanges at KP = 2 .. 128) orders them over compile-time register
// indices, so nothing is indexed dynamically and nothing goes to scratch; then the window
// t <= j < K - t is summed in ascending order and divided.  No LDS, no atomics, no workspace.
//
// Keys.  An fp32 value maps to an unsigned key whose integer order is np.sort's order of the
// values: the sign bit of a positive value is flipped, every bit of a negative one, and a NaN of
// either sign becomes all-ones.  A compare-exchange is then one unsigned min and one unsigned max,
// NaN needs no case of its own in the network, and the padding keys (all-ones too) sit above the
// window by construction.  -0.0 sorts directly below +0.0; the sum starts from +0.0, which makes
// that invisible in the result.  Keys map back to values when the window is summed.
//
// bf16 rows.  A bf16 value's key has 16 bits, so in the vector walk two adjacent elements share a
// register and exchange with the packed 16-bit min and max (v_pk_min_u16 / v_pk_max_u16): half the
// VALU work per element, and a lane owns twice the elements for the same registers.  The element
// walk widens on load and uses the 32-bit keys; any correct network gives the same bits.
//
// Registers decide VEC: 128 key registers per lane at most.
//   fp32:  VEC = 4 (16-B loads) up to KP = 32, 2 at KP = 64, 1 at KP = 128
//   bf16:  VEC = 8 (16-B loads) up to KP = 32, 4 at KP = 64, 2 at KP = 128
// Data movement.  Every row is read once with non-temporal loads.  All K loads of a lane are issued
// before the first key is mapped, in groups of RB_GROUP clients behind one wave-uniform branch each
// (a group reaching past K re-reads row K - 1; the key it would give is replaced by the padding), so
// the memory system sees the whole column of an element at once.  A lane stores VEC * 4 bytes,
// contiguous across the wave.  The vector walk and the element walk are two launches of the same
// kernel template: the second takes the last M % VEC elements, or every element of a call whose
// rows or output are not 16-B aligned.
//
// Arithmetic: acc = +0.0; acc = fl32(acc + v) over the window in ascending order; fl32(acc / n), the
// compiler's correctly rounded fp32 division with denormals kept.  A NaN result is written as the one
// quiet NaN 0x7FC00000, so the two key widths and the two walks agree in every bit.  Compiled with
// -ffp-contract=off and the kernel carries `#pragma clang fp contract(off)`.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "fedagg_robust.h"
#include "lib_error.h"

#define RB_THREADS 256  // threads per workgroup
#define RB_GROUP 8      // clients per load group (one wave-uniform branch each)
#define RB_GRID_X (1u << 24)  // workgroups along x; more tiles than that continue along y
#define RB_VEC_F32 4    // elements per lane of the vector walk up to KP = 32
#define RB_VEC_BF16 8

namespace {

using fedagg_lib_error::fail;
constexpr auto check_launch = fedagg_lib_error::check_launch<FEDAGG_OK, FEDAGG_EHIP>;

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t ONES = 0xFFFFFFFFu;  // the key of a NaN and of the padding
constexpr uint32_t QNAN = 0x7FC00000u;  // every NaN result

struct RbArgs {
  const void* row[FEDAGG_ROBUST_MAX_K];
};

// fp32 bits to the sortable key and back.
__device__ __forceinline__ uint32_t key32(const uint32_t u) {
  const uint32_t k = u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
  return (u & 0x7FFFFFFFu) > 0x7F800000u ? ONES : k;
}

__device__ __forceinline__ float value32(const uint32_t k) {
  return __uint_as_float(k ^ (~(uint32_t)((int32_t)k >> 31) | 0x80000000u));  // all-ones gives a NaN
}

// bf16 bits (in the low half of h) to the 16-bit key and back to the widened value.
__device__ __forceinline__ uint32_t key16(const uint32_t h) {
  const uint32_t k = (h & 0x8000u) ? (~h & 0xFFFFu) : (h | 0x8000u);
  return (h & 0x7FFFu) > 0x7F80u ? 0xFFFFu : k;
}

__device__ __forceinline__ float value16(const uint32_t k) {
  const uint32_t h = (k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xFFFFu);
  return __uint_as_float(h << 16);
}

// One lane's BYTES of a row into its registers, read once: non-temporal.
template <int BYTES>
__device__ __forceinline__ void load_words(const uint8_t* p, uint32_t (&w)[(BYTES + 3) / 4]) {
  if constexpr (BYTES == 16) {
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
  } else if constexpr (BYTES == 8) {
    const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
    w[0] = v[0]; w[1] = v[1];
  } else if constexpr (BYTES == 4) {
    w[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
  } else {
    static_assert(BYTES == 2, "a lane loads 2, 4, 8 or 16 bytes of a row");
    w[0] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p));
  }
}

// The compare-exchange: the smaller key to a, the larger to b (PACK: in each 16-bit half).
template <bool PACK>
__device__ __forceinline__ void exchange(uint32_t& a, uint32_t& b) {
  if constexpr (PACK) {
    const u16x2 x = __builtin_bit_cast(u16x2, a), y = __builtin_bit_cast(u16x2, b);
    a = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(x, y));
    b = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(x, y));
  } else {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
  }
}

// Batcher's odd-even merge sort (Knuth's merge exchange, 5.2.2 M) over r[0 .. KP), KP a power of
// two, ascending.  Every loop bound is a compile-time constant once the loops around it are
// unrolled, so every exchange names two fixed registers.
template <int KP, int NR, bool PACK>
__device__ __forceinline__ void sort_network(uint32_t (&r)[KP][NR]) {
#pragma unroll
  for (int p = 1; p < KP; p *= 2) {
#pragma unroll
    for (int k = p; k >= 1; k /= 2) {
#pragma unroll
      for (int j = k % p; j + k < KP; j += 2 * k) {
#pragma unroll
        for (int i = 0; i < k; ++i) {
          if (i + j + k < KP && (i + j) / (2 * p) == (i + j + k) / (2 * p)) {
#pragma unroll
            for (int q = 0; q < NR; ++q) exchange<PACK>(r[i + j][q], r[i + j + k][q]);
          }
        }
      }
    }
  }
}

// Elements [first + u * VEC, first + (u + 1) * VEC) for u < units, one u per lane.  n is
// fl32(K - 2 t).  KIND: FEDAGG_F32 or FEDAGG_BF16; bf16 lanes of two elements and more hold packed
// 16-bit keys.
template <int KIND, int KP, int VEC>
__global__ void __launch_bounds__(RB_THREADS)
    robust_kernel(const RbArgs a, const int K, const int t, const float n, const uint64_t first, const uint64_t units,
                  float* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr bool BF = KIND == FEDAGG_BF16;
  constexpr bool PACK = BF && VEC >= 2;
  constexpr int ESZ = BF ? 2 : 4;
  constexpr int NR = PACK ? VEC / 2 : VEC;  // key registers per client
  constexpr int G = KP < RB_GROUP ? KP : RB_GROUP;
  static_assert(VEC * ESZ <= 16 && NR * 4 >= VEC * ESZ, "one load per client and lane");
  const int hi = K - t;
  const uint32_t lane_bytes = threadIdx.x * (VEC * ESZ);  // 32 bits: the loads take a scalar base and this offset
  // One tile per workgroup and no loop: the K row addresses are then read where they are used, a group
  // at a time, instead of being held in scalar registers across iterations (there are not that many).
  const uint64_t tile = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (tile * RB_THREADS + threadIdx.x < units) {
    const uint64_t t0 = first + tile * RB_THREADS * VEC;  // the tile's first element: wave-uniform
    uint32_t r[KP][NR];
    // every load of the lane, ahead of the first use
#pragma unroll
    for (int g = 0; g < KP; g += G) {
      if (g < K) {  // wave-uniform
#pragma unroll
        for (int j = g; j < g + G; ++j) {
          const int k = j < K ? j : K - 1;
          load_words<VEC * ESZ>(static_cast<const uint8_t*>(a.row[k]) + t0 * ESZ + lane_bytes, r[j]);
        }
      } else {
#pragma unroll
        for (int j = g; j < g + G; ++j) {
#pragma unroll
          for (int q = 0; q < NR; ++q) r[j][q] = ONES;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < KP; ++j) {
#pragma unroll
      for (int q = 0; q < NR; ++q) {
        const uint32_t w = r[j][q];
        uint32_t key;
        if constexpr (PACK) key = key16(w & 0xFFFFu) | (key16(w >> 16) << 16);
        else key = key32(BF ? w << 16 : w);
        r[j][q] = j < K ? key : ONES;
      }
    }
    sort_network<KP, NR, PACK>(r);
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.0f;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      if (j >= t && j < hi) {  // wave-uniform: the register indices stay static for a runtime t
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          float v;
          if constexpr (PACK) v = value16((e & 1) ? r[j][e / 2] >> 16 : r[j][e / 2] & 0xFFFFu);
          else v = value32(r[j][e]);
          acc[e] = acc[e] + v;
        }
      }
    }
    uint32_t o[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const uint32_t b = __float_as_uint(acc[e] / n);
      o[e] = (b & 0x7FFFFFFFu) > 0x7F800000u ? QNAN : b;  // one NaN, whichever walk and key width made it
    }
    float* dst = out + t0 + threadIdx.x * VEC;
    if constexpr (VEC >= 4) {
#pragma unroll
      for (int q = 0; q < VEC / 4; ++q) {
        const u32x4 v = {o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(dst) + q);
      }
    } else if constexpr (VEC == 2) {
      const u32x2 v = {o[0], o[1]};
      __builtin_nontemporal_store(v, reinterpret_cast<u32x2*>(dst));
    } else {
      dst[0] = __uint_as_float(o[0]);
    }
  }
}

// Elements per lane: the vector walk's by the register budget, the element walk's 1.
constexpr int vec_of(int kind, int kp, bool vector) {
  if (!vector) return 1;
  const int v = kind == FEDAGG_BF16 ? RB_VEC_BF16 : RB_VEC_F32;
  return kp <= 32 ? v : (kp == 64 ? v / 2 : v / 4);
}

struct Call {
  RbArgs a;
  int K, t;
  float n;
  uint64_t first, count;  // the elements this launch covers
  float* out;
  hipStream_t stream;
};

template <int KIND, int KP, bool VECTOR>
void launch(const Call& c) {
  constexpr int VEC = vec_of(KIND, KP, VECTOR);
  const uint64_t units = c.count / VEC;  // the caller passes a multiple of VEC
  const uint64_t tiles = (units + RB_THREADS - 1) / RB_THREADS;  // below 2^36 for M up to 2^44
  const uint64_t gx = tiles < RB_GRID_X ? tiles : RB_GRID_X, gy = (tiles + gx - 1) / gx;
  hipLaunchKernelGGL((robust_kernel<KIND, KP, VEC>), dim3((unsigned)gx, (unsigned)gy), dim3(RB_THREADS), 0, c.stream,
                     c.a, c.K, c.t, c.n, c.first, units, c.out);
}

template <int KIND, bool VECTOR>
void dispatch(const int kp, const Call& c) {
  switch (kp) {
    case 2: return launch<KIND, 2, VECTOR>(c);
    case 4: return launch<KIND, 4, VECTOR>(c);
    case 8: return launch<KIND, 8, VECTOR>(c);
    case 16: return launch<KIND, 16, VECTOR>(c);
    case 32: return launch<KIND, 32, VECTOR>(c);
    case 64: return launch<KIND, 64, VECTOR>(c);
    default: return launch<KIND, 128, VECTOR>(c);
  }
}

}  // namespace

extern "C" {

int fedagg_robust_abi_version(void) { return FEDAGG_ROBUST_ABI_VERSION; }
const char* fedagg_robust_last_error(void) { return fedagg_lib_error::g_error; }

int fedagg_robust_blocking(int* tile_elems, int* vec_f32, int* vec_bf16) {
  if (tile_elems) *tile_elems = RB_THREADS * RB_VEC_BF16;
  if (vec_f32) *vec_f32 = RB_VEC_F32;
  if (vec_bf16) *vec_bf16 = RB_VEC_BF16;
  return FEDAGG_OK;
}

int fedagg_robust_mean(const void* const* d_rows, int kind, int K, int t, uint64_t M, float* d_out, void* stream) {
  if (K <= 0 || K > FEDAGG_ROBUST_MAX_K)
    return fail(FEDAGG_EINVAL, "robust mean: K is outside [1, FEDAGG_ROBUST_MAX_K] (K=%lld)", (long long)K);
  if (t < 0 || 2 * (long long)t >= K)
    return fail(FEDAGG_EINVAL, "robust mean: t must satisfy 0 <= 2 t < K (t=%lld, K=%lld)", (long long)t, (long long)K);
  if (kind != FEDAGG_F32 && kind != FEDAGG_BF16)
    return fail(FEDAGG_EINVAL, "robust mean: kind %lld is not FEDAGG_F32 / FEDAGG_BF16", (long long)kind);
  if (!d_rows) return fail(FEDAGG_EINVAL, "robust mean: d_rows is NULL");
  if (M == 0) return FEDAGG_OK;
  if (M > (1ull << 44)) return fail(FEDAGG_EINVAL, "robust mean: M is too large");
  const uintptr_t esz = kind == FEDAGG_F32 ? 4 : 2;
  uintptr_t low = reinterpret_cast<uintptr_t>(d_out);
  for (int k = 0; k < K; ++k) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(d_rows[k]);
    if (!p) return fail(FEDAGG_EINVAL, "robust mean: row %lld is NULL", (long long)k);
    if (p & (esz - 1)) return fail(FEDAGG_EINVAL, "robust mean: row %lld is not aligned to its element", (long long)k);
    low |= p;
  }
  if (!d_out) return fail(FEDAGG_EINVAL, "robust mean: d_out is NULL");
  if (reinterpret_cast<uintptr_t>(d_out) & 3u) return fail(FEDAGG_EINVAL, "robust mean: d_out is not 4-B aligned");

  int kp = 2;
  while (kp < K) kp *= 2;
  Call c;
  memset(&c.a, 0, sizeof(c.a));
  for (int k = 0; k < K; ++k) c.a.row[k] = d_rows[k];
  c.K = K;
  c.t = t;
  c.n = (float)(K - 2 * t);
  c.out = d_out;
  c.stream = (hipStream_t)stream;
  const uint64_t vec = (uint64_t)vec_of(kind, kp, true);
  const uint64_t mv = (low & 15u) ? 0 : M - M % vec;  // the vector walk's elements
  if (mv) {
    c.first = 0;
    c.count = mv;
    if (kind == FEDAGG_F32) dispatch<FEDAGG_F32, true>(kp, c);
    else dispatch<FEDAGG_BF16, true>(kp, c);
    const int rc = check_launch("robust kernel (vector walk)");
    if (rc) return rc;
  }
  if (mv < M) {
    c.first = mv;
    c.count = M - mv;
    if (kind == FEDAGG_F32) dispatch<FEDAGG_F32, false>(kp, c);
    else dispatch<FEDAGG_BF16, false>(kp, c);
    return check_launch("robust kernel (element walk)");
  }
  return FEDAGG_OK;
}

}  // extern "C"
