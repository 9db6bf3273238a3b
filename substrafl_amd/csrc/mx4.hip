// mx4.hip -- libfedagg_mx4.so (include/fedagg_mx4.h): FedAvg over OCP MXFP4 client rows (4-bit
// e2m1 codes, two to a byte, one e8m0 scale byte per 32 elements) and the quantiser that produces
// such rows, with or without error feedback.
//
// The reduction.  A lane's 16-B non-temporal load is 32 codes of one client, exactly one scale
// block: one scale byte per lane and load, 64 consecutive scale bytes per wave.  MX4_U clients are
// loaded ahead of the in-order add chain (two register buffers), and the 32 fp32 results of a lane
// (128 B) are transposed through 8 KiB of LDS per wave so that every store instruction of a wave
// writes one contiguous 1 KiB run.
//
// Arithmetic per element and client, three roundings that stay three:
//   x = fl32(v * 2^(s-127))     the decode: exact, or overflow to +-inf
//   p = fl32(x * w_k)
//   acc = fl32(acc + p)         client order, from +0.0
// The file is compiled with -ffp-contract=off and every kernel body and helper carries
// `#pragma clang fp contract(off)`.  fp32 denormals are kept: a decoded element may be 2^-128.
//
// At half a byte per element the instructions per byte double, so the walk spends 2.5 VALU
// operations per element where mx.hip spends 3.5: v_cvt_scalef32_pk_f32_fp4 takes the block's scale
// in its scale operand and yields two decoded elements (half an operation each), then one multiply
// by the weight and one add.  The scale operand is the fp32 with the exponent field s, used only
// for s in [2, 252]: there it is the normal number 2^(s-127) and every product is a normal fp32
// (0.5 * 2^-125 up to 6 * 2^125), so nothing rests on what the instruction does with a subnormal or
// non-finite scale or result.  A lane whose scale byte is outside that range (0, 1, 253, 254, 255:
// never produced for ordinary data) converts with the scale operand 1.0 and multiplies by the scale
// constructed from s as mx.hip does; when no lane of the wave has one the branch is skipped.
//
// Two decoders, held to each other and to wire.py by the exhaustive test:
//   - the vector walk: the instruction above;
//   - plain C++ (the tail elements, an unaligned d_out and the numel == 1 kernel): integer nibble
//     extraction, a constant table of the 8 magnitudes in halves, and two multiplies by powers of
//     two, the first of them exact by construction.
//
// The quantiser.  One kernel template, the residual a compile-time flag.  A lane owns 8 consecutive
// elements (two 16-B loads of fp32, one of bf16), the 4 lanes of a quad one scale block.  The block
// maximum is the maximum of the magnitudes' bit patterns in the lane, then the two xor steps over
// the quad as DPP quad permutes: no LDS, no atomics.  Rounding to e2m1 is integer arithmetic, the
// formulas of wire.py.  Each lane writes its 8 codes as one 4-byte store, the quad's first lane the
// scale byte; with the residual the lane also loads and stores 8 fp32 residuals.  The last M % 32
// elements, and the whole call when a pointer lacks the vector walk's alignment, go one element
// per lane (32 lanes a block, pairs of lanes a byte) through the same helpers: identical bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "fedagg_mx4.h"
#include "lib_error.h"
#include "pairwise_sum.h"

#define MX4_THREADS 256  // threads per workgroup
#define MX4_VEC 32       // elements per lane and load: 16 B of codes, one scale block
#define MX4_U 4          // clients per load group (k_group)
#define MX4_TILE (MX4_THREADS * MX4_VEC)  // elements per workgroup step (tile_elems)
#define MX4_PW_IDX 64    // numel == 1 elements per launch of the pairwise kernel
#define MX4_GRID_CAP (1u << 18)
#define MX4_Q_LANE 8                             // elements per lane of the quantiser's vector walk
#define MX4_Q_TILE (MX4_THREADS * MX4_Q_LANE)    // elements per workgroup step of it
#define MX4_Q_GRID 2048u                         // workgroups of the quantiser at most

namespace {

using fedagg_internal::pw_leaf;
using fedagg_lib_error::fail;
constexpr auto check_launch = fedagg_lib_error::check_launch<FEDAGG_OK, FEDAGG_EHIP>;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t QNAN = 0x7FC00000u;
constexpr uint32_t HALVES = 0xC8643210u;  // the 8 magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 in halves, 4 bits each

// 2^(s-127) as the fp32 it is: s == 0 is the subnormal 2^-127; s == 255 poisons the block.
__device__ __forceinline__ float scale_of(uint32_t s) {
  uint32_t b = s << 23;
  if (s == 0) b = 0x00400000u;  // 2^22 * 2^-149
  if (s == 255) b = QNAN;
  return __uint_as_float(b);
}

// Plain C++ decode of the 4-bit code c under the scale byte s: the magnitude is q * 2^p with q <= 12
// halves and p = s - 128 in [-128, 126].  2^p is split into a small factor (q * 2^pb is exact) and
// one in the normal range, so the single rounding is that of the last multiply: exact where
// q * 2^p is an fp32 value (subnormals included), +-inf above.
__device__ __forceinline__ float decode_elem(uint32_t c, uint32_t s) {
#pragma clang fp contract(off)
  if (s == 255u) return __uint_as_float(QNAN);
  const int q = (int)((HALVES >> (4u * (c & 7u))) & 15u);
  const int p = (int)s - 128;
  const int pa = p < -126 ? -126 : p;
  const int pb = p - pa;  // in [-2, 0]
  const float small = (float)q * __uint_as_float((uint32_t)(pb + 127) << 23);
  const float v = small * __uint_as_float((uint32_t)(pa + 127) << 23);
  return (c & 8u) ? -v : v;
}

// The 4-bit code of element i of a packed row: the low nibble first.
__device__ __forceinline__ uint32_t nibble(const uint8_t* row, uint64_t i) {
  const uint32_t b = row[i >> 1];
  return (i & 1) ? b >> 4 : b & 15u;
}

// The 8 codes of one dword under the scale operand f: byte j holds elements 2 j (bits 3:0) and 2 j + 1.
#define MX4_CVT8(dw, f, x)                                                             \
  do {                                                                                 \
    const f32x2 p0_ = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4((dw), (f), 0);          \
    const f32x2 p1_ = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4((dw), (f), 1);          \
    const f32x2 p2_ = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4((dw), (f), 2);          \
    const f32x2 p3_ = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4((dw), (f), 3);          \
    (x)[0] = p0_[0]; (x)[1] = p0_[1]; (x)[2] = p1_[0]; (x)[3] = p1_[1];                \
    (x)[4] = p2_[0]; (x)[5] = p2_[1]; (x)[6] = p3_[0]; (x)[7] = p3_[1];                \
  } while (0)

// acc[j] = fl32(acc[j] + fl32(x_j * w)) over the 32 codes of one 16-B load under the scale byte s.
__device__ __forceinline__ void accumulate_block(const u32x4 raw, const uint32_t s, const float w,
                                                 float (&acc)[MX4_VEC]) {
#pragma clang fp contract(off)
  if (s - 2u <= 250u) {  // s in [2, 252]: the scale in the instruction, every result a normal fp32
    const float f = __uint_as_float(s << 23);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      float x[8];
      MX4_CVT8(raw[d], f, x);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = x[j] * w;               // fl(x_k * w_k), after the decode's own rounding
        acc[8 * d + j] = acc[8 * d + j] + p;    // fl(acc + p), client order
      }
    }
  } else {  // 0, 1, 253, 254, 255: subnormal results, overflow, the NaN block
    const float f = scale_of(s);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      float x[8];
      MX4_CVT8(raw[d], 1.0f, x);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xs = x[j] * f;
        const float p = xs * w;
        acc[8 * d + j] = acc[8 * d + j] + p;
      }
    }
  }
}

struct MxArgs {
  const uint8_t* c[FEDAGG_MX4_KCHUNK];  // code rows
  const uint8_t* s[FEDAGG_MX4_KCHUNK];  // scale rows
  float w[FEDAGG_MX4_KCHUNK];
};

struct MxIdx {
  uint64_t idx[MX4_PW_IDX];
  int n;
};

__device__ __forceinline__ void load_group(const MxArgs& a, const int k, const uint64_t v, u32x4 (&raw)[MX4_U],
                                           uint32_t (&sc)[MX4_U]) {
#pragma unroll
  for (int u = 0; u < MX4_U; ++u) {
    raw[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.c[k + u]) + v);
    sc[u] = a.s[k + u][v];  // 32 elements are one block
  }
}

__device__ __forceinline__ void accumulate(const u32x4 (&raw)[MX4_U], const uint32_t (&sc)[MX4_U], const float* w,
                                           float (&acc)[MX4_VEC]) {
#pragma unroll
  for (int u = 0; u < MX4_U; ++u) accumulate_block(raw[u], sc[u], w[u], acc);
}

// acc[:] = the K clients in order over block v; groups of MX4_U clients are loaded one group ahead
// of the add chain (two register buffers), the last K % MX4_U clients one by one.
__device__ __forceinline__ void reduce_block(const MxArgs& a, const int K, const int first, const uint64_t v,
                                             float (&acc)[MX4_VEC], const float* out) {
#pragma clang fp contract(off)
  if (first) {
#pragma unroll
    for (int j = 0; j < MX4_VEC; ++j) acc[j] = 0.0f;  // NumPy seeds add.reduce with +0.0
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const u32x4 r = reinterpret_cast<const u32x4*>(out + v * MX4_VEC)[q];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[4 * q + j] = __uint_as_float(r[j]);
    }
  }
  int k = 0;
  if (K >= MX4_U) {
    u32x4 ra[MX4_U], rb[MX4_U];
    uint32_t sa[MX4_U], sb[MX4_U];
    load_group(a, 0, v, ra, sa);
    for (;;) {
      const bool mb = k + 2 * MX4_U <= K;
      if (mb) load_group(a, k + MX4_U, v, rb, sb);
      accumulate(ra, sa, a.w + k, acc);
      k += MX4_U;
      if (!mb) break;
      const bool ma = k + 2 * MX4_U <= K;
      if (ma) load_group(a, k + MX4_U, v, ra, sa);
      accumulate(rb, sb, a.w + k, acc);
      k += MX4_U;
      if (!ma) break;
    }
  }
  for (; k < K; ++k)
    accumulate_block(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.c[k]) + v), a.s[k][v], a.w[k], acc);
}

__device__ __forceinline__ void store_direct(float* out, const uint64_t v, const float (&acc)[MX4_VEC]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    u32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = __float_as_uint(acc[4 * q + j]);
    __builtin_nontemporal_store(r, reinterpret_cast<u32x4*>(out + v * MX4_VEC) + q);
  }
}

// A wave's 64 lanes each own 128 contiguous output bytes of one 8 KiB run.  Stored directly, every
// store instruction would write 16 B per lane at a 128-B stride.  Through 8 KiB of LDS per wave they
// become eight fully coalesced 1 KiB stores.  Piece q of lane l (16-B piece j = 8 l + q of the run)
// sits at slot 8 l + ((q + l) & 7): the rotation spreads a store instruction's lanes over the LDS
// banks.  All 64 lanes must be active (the caller checks wave-uniformly).
__device__ __forceinline__ void store_coalesced(float* wave_dst, const float (&acc)[MX4_VEC], u32x4* lds_wave) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    u32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = __float_as_uint(acc[4 * q + j]);
    lds_wave[8 * lane + ((q + lane) & 7)] = r;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int j = q * 64 + lane;  // the 16-B piece this lane stores
    const int l = j >> 3;
    const u32x4 r = lds_wave[8 * l + (((j & 7) + l) & 7)];
    __builtin_nontemporal_store(r, reinterpret_cast<u32x4*>(wave_dst) + j);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // WAR before the buffer is reused
  __builtin_amdgcn_wave_barrier();
}

// nvec: whole 32-element blocks taken by the vector walk (M / 32, or 0 when d_out is not 16-B
// aligned); elements from nvec * 32 on go one by one.
__global__ void __launch_bounds__(MX4_THREADS)
    mx4_fedavg_kernel(const MxArgs a, const int K, const int first, const uint64_t nvec, const uint64_t M,
                      float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ u32x4 stage[MX4_THREADS / 64][512];
  u32x4* lds_wave = stage[threadIdx.x / 64];
  for (uint64_t t = blockIdx.x; t * MX4_THREADS < nvec; t += gridDim.x) {
    const uint64_t v = t * MX4_THREADS + threadIdx.x;
    const uint64_t wave_base = v - (threadIdx.x & 63);
    const bool wave_full = wave_base + 63 < nvec;  // wave-uniform
    if (v < nvec) {
      float acc[MX4_VEC];
      reduce_block(a, K, first, v, acc, out);
      if (wave_full) store_coalesced(out + wave_base * MX4_VEC, acc, lds_wave);
      else store_direct(out, v, acc);
    }
  }
  // the last M % 32 elements (everything when d_out is not 16-B aligned): plain C++
  const uint64_t stride = (uint64_t)gridDim.x * MX4_THREADS;
  for (uint64_t i = nvec * MX4_VEC + (uint64_t)blockIdx.x * MX4_THREADS + threadIdx.x; i < M; i += stride) {
    float acc = first ? 0.0f : out[i];
    for (int k = 0; k < K; ++k) {
      const float x = decode_elem(nibble(a.c[k], i), a.s[k][i >> 5]);
      const float p = x * a.w[k];
      acc = acc + p;
    }
    out[i] = acc;
  }
}

// numel == 1 elements: one leaf (n <= 128 terms) of NumPy's pairwise tree over the products of the
// n clients in `a`, one lane per element.  add: the running node value in out[i] is the other
// operand of this node's sum; fin: this is the tree's root, and NumPy's reduction adds it to +0.0.
__global__ void __launch_bounds__(MX4_PW_IDX)
    mx4_pairwise_kernel(const MxArgs a, const MxIdx ix, const int n, const int add, const int fin,
                        float* __restrict__ out) {
#pragma clang fp contract(off)
  if ((int)threadIdx.x >= ix.n) return;
  const uint64_t i = ix.idx[threadIdx.x];
  auto get = [&](int64_t k) -> float {
    const float x = decode_elem(nibble(a.c[k], i), a.s[k][i >> 5]);
    return x * a.w[k];
  };
  float r = pw_leaf<float>(get, 0, n);
  if (add) r = out[i] + r;
  if (fin) r = 0.0f + r;
  out[i] = r;
}

// ------------------------------------------------------------------------------------
// Quantiser
// ------------------------------------------------------------------------------------

// fp32 bits of a finite |y| to the e2m1 magnitude code: nearest even, 6 and above to 7.
__device__ __forceinline__ uint32_t e2m1_of(const uint32_t a) {
#pragma clang fp contract(off)
  if (a >= 0x40C00000u) return 7u;  // 6
  if (a < 0x3F800000u) {            // below 1 the values are the multiples of 0.5:
    const float f = __uint_as_float(a) + 4194304.0f;  // 2^22 has ulp 0.5, the add rounds to it
    return __float_as_uint(f) - 0x4A800000u;
  }
  return (a + 0x1FFFFFu + ((a >> 22) & 1u) - 0x3F000000u) >> 22;
}

// The scale byte s = e + 127 of a block whose maximum magnitude has the bits a (finite, not zero),
// and inv = 2^-e, the factor its elements are multiplied by before rounding to e2m1.
__device__ __forceinline__ uint32_t finite_scale(const uint32_t a, float& inv) {
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
  int e = fl - 2;
  if (mant >= 0x00E00000u) e += 1;  // amax * 2^-e >= 7 = 1.75 * 2^2: the tie that would round to 8
  e = e < -127 ? -127 : (e > 127 ? 127 : e);
  const uint32_t f = (uint32_t)(127 - e);            // exponent field of 2^-e
  inv = __uint_as_float(f ? f << 23 : 0x00400000u);  // 2^-127 is a subnormal
  return (uint32_t)(e + 127);
}

// The maximum over the 4 lanes of a quad: quad_perm [1,0,3,2] is lane xor 1, [2,3,0,1] lane xor 2.
__device__ __forceinline__ uint32_t quad_max(uint32_t a) {
  uint32_t o = (uint32_t)__builtin_amdgcn_mov_dpp((int)a, 0xB1, 0xF, 0xF, true);
  a = o > a ? o : a;
  o = (uint32_t)__builtin_amdgcn_mov_dpp((int)a, 0x4E, 0xF, 0xF, true);
  return o > a ? o : a;
}

// What a block's maximum decides: the scale byte, 2^-e for the encode and 2^(s-127) for the decode.
struct BlockScale {
  uint32_t s;
  float inv, f;
  bool bad, zero;  // NaN or Inf in the block; every element +-0
};

__device__ __forceinline__ BlockScale block_scale(const uint32_t a) {
  BlockScale b;
  b.bad = a >= 0x7F800000u;
  b.zero = a == 0u;
  const uint32_t s = finite_scale((b.bad || b.zero) ? 0x3F800000u : a, b.inv);
  b.s = b.bad ? 255u : (b.zero ? 127u : s);
  b.f = scale_of(b.zero ? 127u : s);  // finite also for a bad block: its res' is selected below
  return b;
}

// The 4-bit code of r under the block's scale (a bad block's codes are 0; a zero block's carry the
// signs: +-0 * inv is +-0 and e2m1_of(0) is 0).
__device__ __forceinline__ uint32_t encode(const float r, const BlockScale& b) {
#pragma clang fp contract(off)
  const float y = r * b.inv;
  const uint32_t yu = __float_as_uint(y);
  const uint32_t c = e2m1_of(yu & 0x7FFFFFFFu) | ((yu >> 28) & 8u);
  return b.bad ? 0u : c;
}

// res' from r and the unscaled value v of its code: fl32(r - d) where the block and d are finite,
// +0.0 otherwise (the rule of fedagg_mxef.h).
__device__ __forceinline__ float residual(const float r, const float v, const BlockScale& b) {
#pragma clang fp contract(off)
  const float d = v * b.f;
  const bool fin = (__float_as_uint(d) & 0x7FFFFFFFu) < 0x7F800000u;
  const float e = r - d;
  return (fin && !b.bad) ? e : 0.0f;
}

template <int KIND>
__device__ __forceinline__ void load_x8(const void* __restrict__ x_, const uint64_t i, float (&x)[MX4_Q_LANE]) {
  if constexpr (KIND == FEDAGG_BF16) {
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(x_) + i));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[2 * j] = __uint_as_float(v[j] << 16);
      x[2 * j + 1] = __uint_as_float(v[j] & 0xFFFF0000u);
    }
  } else {
    const u32x4* p = reinterpret_cast<const u32x4*>(static_cast<const uint32_t*>(x_) + i);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const u32x4 v = __builtin_nontemporal_load(p + q);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[4 * q + j] = __uint_as_float(v[j]);
    }
  }
}

// mv: the elements of the vector walk, a multiple of 32 (0 when the pointers lack its alignment);
// elements from mv on go one per lane.  EF: res is the residual, read and rewritten; else unused.
template <int KIND, bool EF>
__global__ void __launch_bounds__(MX4_THREADS)
    mx4_quantize_kernel(const void* __restrict__ x_, const uint64_t mv, const uint64_t M, float* __restrict__ res,
                        uint8_t* __restrict__ codes, uint8_t* __restrict__ scales) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  for (uint64_t t = blockIdx.x; t * MX4_Q_TILE < mv; t += gridDim.x) {
    const uint64_t i = t * MX4_Q_TILE + (uint64_t)threadIdx.x * MX4_Q_LANE;  // this lane's first element
    if (i < mv) {  // mv is a multiple of 32: the 4 lanes of a quad are in range together
      float r[MX4_Q_LANE];
      load_x8<KIND>(x_, i, r);
      u32x4* rp = reinterpret_cast<u32x4*>(res + i);
      if constexpr (EF) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const u32x4 v = __builtin_nontemporal_load(rp + q);
#pragma unroll
          for (int j = 0; j < 4; ++j) r[4 * q + j] = r[4 * q + j] + __uint_as_float(v[j]);
        }
      }
      uint32_t a = 0;
#pragma unroll
      for (int j = 0; j < MX4_Q_LANE; ++j) {
        const uint32_t mag = __float_as_uint(r[j]) & 0x7FFFFFFFu;
        a = mag > a ? mag : a;
      }
      const BlockScale b = block_scale(quad_max(a));
      uint32_t c = 0;
#pragma unroll
      for (int j = 0; j < MX4_Q_LANE; ++j) c |= encode(r[j], b) << (4 * j);
      *reinterpret_cast<uint32_t*>(codes + (i >> 1)) = c;
      if ((lane & 3) == 0) scales[i >> 5] = (uint8_t)b.s;
      if constexpr (EF) {
        float v[8];
        MX4_CVT8(c, 1.0f, v);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          u32x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = __float_as_uint(residual(r[4 * q + j], v[4 * q + j], b));
          __builtin_nontemporal_store(o, rp + q);
        }
      }
    }
  }

  // one element per lane from mv on; every lane of a block walks the same steps
  const uint64_t padded = (M + 31) & ~(uint64_t)31;
  const uint64_t stride = (uint64_t)gridDim.x * MX4_THREADS;
  for (uint64_t i = mv + (uint64_t)blockIdx.x * MX4_THREADS + threadIdx.x; i < padded; i += stride) {
    float r = 0.0f;  // lanes past M hold +0: no effect on the maximum, and their code is 0
    if (i < M) {
      if constexpr (KIND == FEDAGG_BF16) r = __uint_as_float((uint32_t)static_cast<const uint16_t*>(x_)[i] << 16);
      else r = static_cast<const float*>(x_)[i];
      if constexpr (EF) r = r + res[i];
    }
    uint32_t a = __float_as_uint(r) & 0x7FFFFFFFu;
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)a, d, 32);
      a = o > a ? o : a;
    }
    const BlockScale b = block_scale(a);
    const uint32_t c = encode(r, b);
    const uint32_t hi = (uint32_t)__shfl_xor((int)c, 1, 32);  // the odd neighbour's code: the byte's high nibble
    if (i < M) {
      if ((i & 1) == 0) codes[i >> 1] = (uint8_t)(c | (hi << 4));
      if ((i & 31) == 0) scales[i >> 5] = (uint8_t)b.s;
      if constexpr (EF) {
        const f32x2 v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c, 1.0f, 0);
        res[i] = residual(r, v[0], b);
      }
    }
  }
}

unsigned grid_for(uint64_t work_items, uint64_t per_block, uint64_t cap) {
  uint64_t g = (work_items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return (unsigned)(g > cap ? cap : g);
}

void fill_args(MxArgs& a, const uint8_t* const* codes, const uint8_t* const* scales, const float* w, int k0, int n) {
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < n; ++k) {
    a.c[k] = codes[k0 + k];
    a.s[k] = scales[k0 + k];
    a.w[k] = w[k0 + k];
  }
}

bool overlap(const void* p, uint64_t np, const void* q, uint64_t nq) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + nq && b < a + np;
}

template <int KIND, bool EF>
void launch_quantize(unsigned grid, hipStream_t stream, const void* d_x, uint64_t mv, uint64_t M, float* d_res,
                     uint8_t* d_codes, uint8_t* d_scales) {
  hipLaunchKernelGGL((mx4_quantize_kernel<KIND, EF>), dim3(grid), dim3(MX4_THREADS), 0, stream, d_x, mv, M, d_res,
                     d_codes, d_scales);
}

}  // namespace

extern "C" {

int fedagg_mx4_abi_version(void) { return FEDAGG_MX4_ABI_VERSION; }
const char* fedagg_mx4_last_error(void) { return fedagg_lib_error::g_error; }

int fedagg_mx4_blocking(int* tile_elems, int* k_group) {
  if (tile_elems) *tile_elems = MX4_TILE;
  if (k_group) *k_group = MX4_U;
  return FEDAGG_OK;
}

int fedagg_mx4_fedavg_e2m1(const uint8_t* const* d_codes, const uint8_t* const* d_scales, const float* h_w, int K,
                           uint64_t M, const uint64_t* h_idx, int P, float* d_out, void* stream) {
  if (K <= 0) return fail(FEDAGG_EINVAL, "mx4 fedavg: K must be positive (K=%lld)", (long long)K);
  if (!d_codes) return fail(FEDAGG_EINVAL, "mx4 fedavg: d_codes is NULL");
  if (!d_scales) return fail(FEDAGG_EINVAL, "mx4 fedavg: d_scales is NULL");
  if (!h_w) return fail(FEDAGG_EINVAL, "mx4 fedavg: h_w is NULL");
  if (P < 0) return fail(FEDAGG_EINVAL, "mx4 fedavg: P is negative (P=%lld)", (long long)P);
  if (P > 0 && !h_idx) return fail(FEDAGG_EINVAL, "mx4 fedavg: h_idx is NULL with P > 0");
  if (M == 0) return FEDAGG_OK;
  if (M > (1ull << 44)) return fail(FEDAGG_EINVAL, "mx4 fedavg: M is too large");
  for (int k = 0; k < K; ++k) {
    if (!d_codes[k]) return fail(FEDAGG_EINVAL, "mx4 fedavg: code row %lld is NULL", (long long)k);
    if (reinterpret_cast<uintptr_t>(d_codes[k]) & 15u)
      return fail(FEDAGG_EINVAL, "mx4 fedavg: code row %lld is not 16-B aligned", (long long)k);
    if (!d_scales[k]) return fail(FEDAGG_EINVAL, "mx4 fedavg: scale row %lld is NULL", (long long)k);
  }
  if (!d_out) return fail(FEDAGG_EINVAL, "mx4 fedavg: d_out is NULL");
  if (reinterpret_cast<uintptr_t>(d_out) & 3u) return fail(FEDAGG_EINVAL, "mx4 fedavg: d_out is not 4-B aligned");
  for (int p = 0; p < P; ++p)
    if (h_idx[p] >= M) return fail(FEDAGG_EINVAL, "mx4 fedavg: numel == 1 index %lld is out of range", (long long)p);
  if (P > 0 && K > FEDAGG_MX4_MAX_PAIRWISE_K)
    return fail(FEDAGG_EINVAL, "mx4 fedavg: numel == 1 elements are served up to FEDAGG_MX4_MAX_PAIRWISE_K clients (K=%lld)", (long long)K);

  const uint64_t nvec = (reinterpret_cast<uintptr_t>(d_out) & 15u) ? 0 : M / MX4_VEC;
  const unsigned grid = nvec ? grid_for(M, MX4_TILE, MX4_GRID_CAP) : grid_for(M, MX4_THREADS, MX4_GRID_CAP);
  MxArgs a;
  for (int k0 = 0; k0 < K; k0 += FEDAGG_MX4_KCHUNK) {
    const int n = K - k0 < FEDAGG_MX4_KCHUNK ? K - k0 : FEDAGG_MX4_KCHUNK;
    fill_args(a, d_codes, d_scales, h_w, k0, n);
    hipLaunchKernelGGL(mx4_fedavg_kernel, dim3(grid), dim3(MX4_THREADS), 0, (hipStream_t)stream, a, n, k0 == 0 ? 1 : 0,
                       nvec, M, d_out);
    const int rc = check_launch("mx4 fedavg kernel");
    if (rc) return rc;
  }
  if (P == 0) return FEDAGG_OK;

  // NumPy's pairwise tree over the K products (a leaf up to 128 terms, else split at n / 2 rounded
  // down to a multiple of 8).  Up to 256 terms every inner node has a leaf child, so a node's value
  // waits in d_out[i] for that leaf and nothing else is pending (IEEE addition commutes, so which
  // operand waits does not matter).
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
  for (int p0 = 0; p0 < P; p0 += MX4_PW_IDX) {
    MxIdx ix;
    memset(&ix, 0, sizeof(ix));
    ix.n = P - p0 < MX4_PW_IDX ? P - p0 : MX4_PW_IDX;
    for (int p = 0; p < ix.n; ++p) ix.idx[p] = h_idx[p0 + p];
    for (int st = 0; st < nsteps; ++st) {
      fill_args(a, d_codes, d_scales, h_w, steps[st].lo, steps[st].n);
      hipLaunchKernelGGL(mx4_pairwise_kernel, dim3(1), dim3(MX4_PW_IDX), 0, (hipStream_t)stream, a, ix, steps[st].n,
                         steps[st].add, steps[st].fin, d_out);
      const int rc = check_launch("mx4 pairwise kernel");
      if (rc) return rc;
    }
  }
  return FEDAGG_OK;
}

int fedagg_mx4_quantize(const void* d_x, int kind, uint64_t M, float* d_res, uint8_t* d_codes, uint8_t* d_scales,
                        void* stream) {
  if (kind != FEDAGG_F32 && kind != FEDAGG_BF16)
    return fail(FEDAGG_EINVAL, "mx4 quantize: kind %lld is not FEDAGG_F32 / FEDAGG_BF16", (long long)kind);
  if (M == 0) return FEDAGG_OK;
  if (M > (1ull << 44)) return fail(FEDAGG_EINVAL, "mx4 quantize: M is too large");
  const uint64_t esz = kind == FEDAGG_F32 ? 4 : 2;
  if (!d_x) return fail(FEDAGG_EINVAL, "mx4 quantize: d_x is NULL");
  if (reinterpret_cast<uintptr_t>(d_x) & (esz - 1))
    return fail(FEDAGG_EINVAL, "mx4 quantize: d_x is not aligned to its element size");
  if (reinterpret_cast<uintptr_t>(d_res) & 3u) return fail(FEDAGG_EINVAL, "mx4 quantize: d_res is not 4-B aligned");
  if (!d_codes) return fail(FEDAGG_EINVAL, "mx4 quantize: d_codes is NULL");
  if (!d_scales) return fail(FEDAGG_EINVAL, "mx4 quantize: d_scales is NULL");
  const uint64_t nc = (M + 1) / 2, nb = (M + 31) / 32;
  if (d_res) {
    if (overlap(d_res, 4 * M, d_x, esz * M)) return fail(FEDAGG_EINVAL, "mx4 quantize: d_res overlaps d_x");
    if (overlap(d_res, 4 * M, d_codes, nc)) return fail(FEDAGG_EINVAL, "mx4 quantize: d_res overlaps d_codes");
    if (overlap(d_res, 4 * M, d_scales, nb)) return fail(FEDAGG_EINVAL, "mx4 quantize: d_res overlaps d_scales");
  }

  const bool vec = !((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_res)) & 15u) &&
                   !(reinterpret_cast<uintptr_t>(d_codes) & 3u);
  const uint64_t mv = vec ? M & ~(uint64_t)31 : 0;
  const uint64_t steps_v = (mv + MX4_Q_TILE - 1) / MX4_Q_TILE, steps_e = (M - mv + MX4_THREADS - 1) / MX4_THREADS;
  const unsigned g = grid_for(steps_v > steps_e ? steps_v : steps_e, 1, MX4_Q_GRID);
  hipStream_t st = (hipStream_t)stream;
  if (kind == FEDAGG_F32) {
    if (d_res) launch_quantize<FEDAGG_F32, true>(g, st, d_x, mv, M, d_res, d_codes, d_scales);
    else launch_quantize<FEDAGG_F32, false>(g, st, d_x, mv, M, d_res, d_codes, d_scales);
  } else {
    if (d_res) launch_quantize<FEDAGG_BF16, true>(g, st, d_x, mv, M, d_res, d_codes, d_scales);
    else launch_quantize<FEDAGG_BF16, false>(g, st, d_x, mv, M, d_res, d_codes, d_scales);
  }
  return check_launch("mx4 quantize kernel");
}

}  // extern "C"
