// mx_down.hip -- libfedagg_mxdl.so (include/fedagg_mxdl.h): the MXFP8 downlink.  The aggregator's
// average leaves the add chain already encoded (fedagg_mxdl_fedavg), and a client adds the decoded
// average onto its fp32 parameters in one pass (fedagg_mxdl_increment; fedagg_mxdl_decode for a
// bf16 model).  The fp32 average never reaches HBM on either side.
//
// The fused average.  The split is mx.hip's: 256 threads, a lane owns DL_VEC = 16 consecutive
// elements (one 16-B non-temporal code load per client for e4m3 rows, one 8-B load for packed e2m1
// rows), DL_U clients are loaded one group ahead of the in-order add chain.  Arithmetic per
// element and client, three roundings that stay three:
//   x = fl32(v * 2^(s-127));  p = fl32(x * w_k);  acc = fl32(acc + p)     client order, from +0.0
// (-ffp-contract=off, `#pragma clang fp contract(off)` in every body, packed fp32 instructions off).
// After the chain a lane holds half a scale block in registers, its neighbour (lane xor 1) the
// other half:
//   maximum the in-lane maximum of the 16 magnitude bit patterns, then ONE DPP quad permute with
//           lane xor 1: no LDS, no atomics; NaN and Inf sort above every finite value
//   encode  block_scale / encode of mx_codec.h, the bits of mx.hip's quantiser; a non-finite or
//           all-zero block takes the same instructions and is selected at the end, so no lane
//           pair diverges
//   stores  the 16 codes of a lane as ONE 16-B store, so a wave writes 1 KiB contiguous and the
//           LDS transposition of mx.hip's fp32 output is not needed; the wave's 32 scale bytes
//           are collected through 32 bytes of LDS and leave as two 16-B stores when the scale row
//           is 16-B aligned and the wave is whole, as byte stores from the even lanes otherwise.
//           Plain vector-unit stores only.
// The walk runs over 2 * ceil(M / 32) lane vectors, so both lanes of the last block are there:
// one that owns no element contributes +0 to the maximum, one that owns fewer than 16 takes its
// elements one by one through the plain C++ decoders (exact, like the instructions: same bits).
// An output code pointer that is not 16-B aligned changes only the store, to bytes.
//
// numel == 1 elements.  A second small kernel, one 32-lane group per block that holds a listed
// index: every lane recomputes its element (the listed ones with pw_leaf, NumPy's tree over
// K <= 128 terms, the others sequentially as above), the group exchanges the maximum and rewrites
// the block's 32 codes and its scale byte.
//
// The increment.  A lane owns 16 flat elements of the concatenated tensors (half a block, one scale
// byte).  Where they lie inside one tensor: one 16-B code load, v_cvt_pk_f32_fp8 times the scale,
// and 16-B loads and stores of w from the lane's first 16-B aligned address (up to 3 single
// elements before and after, so a tensor whose flat offset is no multiple of 4 -- any tensor after
// a bias of 1 or 10 -- still moves in vectors).  Elsewhere (tensor boundaries, the tail, a
// misaligned code pointer): element by element with the same instruction, identical bits.
// Tensors go DL_SEG to a launch; a lane finds its tensor by bisection of the launch's offsets.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fedagg_mxdl.h"
#include "lib_error.h"
#include "mx_codec.h"
#include "pairwise_sum.h"

#define DL_THREADS 256  // threads per workgroup
#define DL_VEC 16       // elements per lane: half a scale block (lane_elems)
#define DL_U 4          // clients per load group (k_group)
#define DL_TILE (DL_THREADS * DL_VEC)  // elements per workgroup step (tile_elems)
#define DL_PW_BLOCKS 64  // blocks per launch of the numel == 1 kernel
#define DL_SEG 32        // tensors per launch of the increment
#define DL_GRID_CAP (1u << 18)

namespace {

using fedagg_internal::block_scale;
using fedagg_internal::BlockScale;
using fedagg_internal::decode_elem;
using fedagg_internal::encode;
using fedagg_internal::pw_leaf;
using fedagg_internal::QNAN;
using fedagg_internal::scale_of;
using fedagg_lib_error::fail;
constexpr auto check_launch = fedagg_lib_error::check_launch<FEDAGG_OK, FEDAGG_EHIP>;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int E4M3 = FEDAGG_MXDL_E4M3, E2M1 = FEDAGG_MXDL_E2M1;
constexpr uint32_t HALVES = 0xC8643210u;  // the 8 e2m1 magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 in halves, 4 bits each

struct MxArgs {
  const uint8_t* c[FEDAGG_MXDL_KMAX];  // code rows
  const uint8_t* s[FEDAGG_MXDL_KMAX];  // scale rows
  float w[FEDAGG_MXDL_KMAX];
};

// ------------------------------------------------------------------------------------
// Decoders.  Every decode is exact (or overflows to +-inf), so the instruction forms and the plain
// C++ forms give the same bits, and those of mx.hip and mx4.hip.
// ------------------------------------------------------------------------------------

// Plain C++ decode of the 4-bit e2m1 code c under the scale byte s (mx4.hip's): the magnitude is
// q * 2^p with q <= 12 halves and p = s - 128; 2^p is split so that the single rounding is that of
// the last multiply.
__device__ __forceinline__ float decode_elem4(uint32_t c, uint32_t s) {
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

// Element i of client row `row` under the scale byte s, plain C++.
template <int KIND>
__device__ __forceinline__ float decode_one(const uint8_t* row, const uint64_t i, const uint32_t s) {
  if constexpr (KIND == E4M3) {
    return decode_elem(row[i], s);
  } else {
    const uint32_t b = row[i >> 1];  // the low nibble first
    return decode_elem4((i & 1) ? b >> 4 : b & 15u, s);
  }
}

// What a lane loads of one client: 16 codes.
template <int KIND>
struct Raw {
  typedef u32x4 type;
};
template <>
struct Raw<E2M1> {
  typedef u32x2 type;
};

template <int KIND>
__device__ __forceinline__ typename Raw<KIND>::type load_raw(const uint8_t* row, const uint64_t v) {
  return __builtin_nontemporal_load(reinterpret_cast<const typename Raw<KIND>::type*>(row) + v);
}

// The 8 e2m1 codes of one dword under the scale operand f: byte j holds elements 2 j (bits 3:0) and 2 j + 1.
#define DL_CVT8(dw, f, x)                                                              \
  do {                                                                                 \
    const f32x2 p0_ = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4((dw), (f), 0);          \
    const f32x2 p1_ = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4((dw), (f), 1);          \
    const f32x2 p2_ = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4((dw), (f), 2);          \
    const f32x2 p3_ = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4((dw), (f), 3);          \
    (x)[0] = p0_[0]; (x)[1] = p0_[1]; (x)[2] = p1_[0]; (x)[3] = p1_[1];                \
    (x)[4] = p2_[0]; (x)[5] = p2_[1]; (x)[6] = p3_[0]; (x)[7] = p3_[1];                \
  } while (0)

// The 4 e4m3 codes of one dword times the scale f.
__device__ __forceinline__ void decode_dword(const uint32_t dw, const float f, float (&x)[4]) {
#pragma clang fp contract(off)
  const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)dw, false);  // bytes 0, 1
  const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)dw, true);   // bytes 2, 3
  x[0] = lo[0] * f;
  x[1] = lo[1] * f;
  x[2] = hi[0] * f;
  x[3] = hi[1] * f;
}

// acc[j] = fl32(acc[j] + fl32(x_j * w)) over the 16 codes of one load under the scale byte s.
__device__ __forceinline__ void accumulate_raw(const u32x4 raw, const uint32_t s, const float w, float (&acc)[DL_VEC]) {
#pragma clang fp contract(off)
  const float f = scale_of(s);
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    float x[4];
    decode_dword(raw[d], f, x);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p = x[j] * w;             // fl(x_k * w_k), after the decode's own rounding
      acc[4 * d + j] = acc[4 * d + j] + p;  // fl(acc + p), client order
    }
  }
}

// The e2m1 form, the one of mx4.hip: the scale rides in the instruction's scale operand for s in
// [2, 252], where every result is a normal fp32; a lane whose scale byte is outside (0, 1, 253,
// 254, 255) converts under 1.0 and multiplies by the scale constructed from s.
__device__ __forceinline__ void accumulate_raw(const u32x2 raw, const uint32_t s, const float w, float (&acc)[DL_VEC]) {
#pragma clang fp contract(off)
  if (s - 2u <= 250u) {
    const float f = __uint_as_float(s << 23);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      float x[8];
      DL_CVT8(raw[d], f, x);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = x[j] * w;
        acc[8 * d + j] = acc[8 * d + j] + p;
      }
    }
  } else {
    const float f = scale_of(s);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      float x[8];
      DL_CVT8(raw[d], 1.0f, x);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xs = x[j] * f;
        const float p = xs * w;
        acc[8 * d + j] = acc[8 * d + j] + p;
      }
    }
  }
}

template <int KIND>
__device__ __forceinline__ void load_group(const MxArgs& a, const int k, const uint64_t v,
                                           typename Raw<KIND>::type (&raw)[DL_U], uint32_t (&sc)[DL_U]) {
#pragma unroll
  for (int u = 0; u < DL_U; ++u) {
    raw[u] = load_raw<KIND>(a.c[k + u], v);
    sc[u] = a.s[k + u][v >> 1];  // 16 elements are half a block
  }
}

template <int KIND>
__device__ __forceinline__ void accumulate(const typename Raw<KIND>::type (&raw)[DL_U], const uint32_t (&sc)[DL_U],
                                           const float* w, float (&acc)[DL_VEC]) {
#pragma unroll
  for (int u = 0; u < DL_U; ++u) accumulate_raw(raw[u], sc[u], w[u], acc);
}

// acc[:] += the K clients in order over the whole lane vector v; groups of DL_U clients are loaded
// one group ahead of the add chain (two register buffers), the last K % DL_U clients one by one.
template <int KIND>
__device__ __forceinline__ void reduce_vector(const MxArgs& a, const int K, const uint64_t v, float (&acc)[DL_VEC]) {
  int k = 0;
  if (K >= DL_U) {
    typename Raw<KIND>::type ra[DL_U], rb[DL_U];
    uint32_t sa[DL_U], sb[DL_U];
    load_group<KIND>(a, 0, v, ra, sa);
    for (;;) {
      const bool mb = k + 2 * DL_U <= K;
      if (mb) load_group<KIND>(a, k + DL_U, v, rb, sb);
      accumulate<KIND>(ra, sa, a.w + k, acc);
      k += DL_U;
      if (!mb) break;
      const bool ma = k + 2 * DL_U <= K;
      if (ma) load_group<KIND>(a, k + DL_U, v, ra, sa);
      accumulate<KIND>(rb, sb, a.w + k, acc);
      k += DL_U;
      if (!ma) break;
    }
  }
  for (; k < K; ++k) accumulate_raw(load_raw<KIND>(a.c[k], v), a.s[k][v >> 1], a.w[k], acc);
}

// The same over the first n < 16 elements of lane vector v (the row ends inside it), plain C++.
template <int KIND>
__device__ __forceinline__ void reduce_elements(const MxArgs& a, const int K, const uint64_t v, const int n,
                                                float (&acc)[DL_VEC]) {
#pragma clang fp contract(off)
  for (int k = 0; k < K; ++k) {
    const uint32_t s = a.s[k][v >> 1];
    const float w = a.w[k];
#pragma unroll
    for (int j = 0; j < DL_VEC; ++j) {
      if (j < n) {
        const float p = decode_one<KIND>(a.c[k], v * DL_VEC + j, s) * w;
        acc[j] = acc[j] + p;
      }
    }
  }
}

// The maximum of a lane and its neighbour lane xor 1: quad_perm [1,0,3,2].
__device__ __forceinline__ uint32_t pair_max(const uint32_t a) {
  const uint32_t o = (uint32_t)__builtin_amdgcn_mov_dpp((int)a, 0xB1, 0xF, 0xF, true);
  return o > a ? o : a;
}

// nfull: lane vectors that lie wholly inside the row (M / 16).  codes16 / scales16: the output
// pointer is 16-B aligned.
template <int KIND>
__global__ void __launch_bounds__(DL_THREADS)
    mxdl_fedavg_kernel(const MxArgs a, const int K, const uint64_t M, uint8_t* __restrict__ codes,
                       uint8_t* __restrict__ scales, const int codes16, const int scales16) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) uint8_t sc_stage[DL_THREADS / 64][32];
  const int lane = threadIdx.x & 63;
  uint8_t* sc_wave = sc_stage[threadIdx.x / 64];
  const uint64_t nfull = M / DL_VEC;
  const uint64_t nvec = 2 * ((M + 31) / 32);  // both lanes of every block, the last partial one included

  for (uint64_t t = blockIdx.x; t * DL_THREADS < nvec; t += gridDim.x) {
    const uint64_t v = t * DL_THREADS + threadIdx.x;
    const uint64_t wave_v = v - lane;
    const bool wide_scales = scales16 && wave_v + 64 <= nfull;  // wave-uniform: all 64 lanes hold whole vectors
    if (v < nvec) {  // nvec is even: the two lanes of a block are in range together
      const int n = v < nfull ? DL_VEC : (M > v * DL_VEC ? (int)(M - v * DL_VEC) : 0);  // elements this lane owns
      float acc[DL_VEC];
#pragma unroll
      for (int j = 0; j < DL_VEC; ++j) acc[j] = 0.0f;  // NumPy seeds add.reduce with +0.0; a lane past M keeps +0
      if (n == DL_VEC) reduce_vector<KIND>(a, K, v, acc);
      else if (n > 0) reduce_elements<KIND>(a, K, v, n, acc);

      uint32_t amax = 0;
#pragma unroll
      for (int j = 0; j < DL_VEC; ++j) {
        const uint32_t mag = __float_as_uint(acc[j]) & 0x7FFFFFFFu;
        amax = mag > amax ? mag : amax;
      }
      const BlockScale b = block_scale(pair_max(amax));
      u32x4 c;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) w |= encode(acc[4 * q + j], b) << (8 * j);
        c[q] = w;
      }
      if (n == DL_VEC && codes16) {
        __builtin_nontemporal_store(c, reinterpret_cast<u32x4*>(codes) + v);
      } else {
#pragma unroll
        for (int j = 0; j < DL_VEC; ++j)
          if (j < n) codes[v * DL_VEC + j] = (uint8_t)(c[j >> 2] >> (8 * (j & 3)));
      }
      if ((lane & 1) == 0) {  // the block's first lane owns at least one element
        if (wide_scales) sc_wave[lane >> 1] = (uint8_t)b.s;
        else scales[v >> 1] = (uint8_t)b.s;
      }
    }
    if (wide_scales) {  // all 64 lanes are here
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (lane < 2)
        reinterpret_cast<u32x4*>(scales + (wave_v >> 1))[lane] = reinterpret_cast<const u32x4*>(sc_wave)[lane];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // WAR before the next step's bytes
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// The blocks that hold numel == 1 elements: mask bit l says element 32 * block + l is one.
struct PwBlocks {
  uint64_t block[DL_PW_BLOCKS];
  uint32_t mask[DL_PW_BLOCKS];
  int n;
};

// One 32-lane group per listed block, one element per lane; K <= 128, so NumPy's tree is one leaf.
template <int KIND>
__global__ void __launch_bounds__(DL_THREADS)
    mxdl_pairwise_kernel(const MxArgs a, const PwBlocks pb, const int K, const uint64_t M, uint8_t* __restrict__ codes,
                         uint8_t* __restrict__ scales) {
#pragma clang fp contract(off)
  const int g = (int)(blockIdx.x * (DL_THREADS / 32) + threadIdx.x / 32);
  const int l = threadIdx.x & 31;
  const bool on = g < pb.n;  // a group past the table walks block 0's steps and stores nothing
  const uint64_t blk = pb.block[on ? g : 0];
  const uint32_t mask = pb.mask[on ? g : 0];
  const uint64_t i = blk * 32 + l;
  float r = 0.0f;  // lanes past M hold +0: no effect on the maximum
  if (i < M) {
    auto get = [&](int64_t k) -> float { return decode_one<KIND>(a.c[k], i, a.s[k][blk]) * a.w[k]; };
    if ((mask >> l) & 1u) {
      r = 0.0f + pw_leaf<float>(get, 0, K);  // NumPy's reduction adds the tree's root to +0.0
    } else {
      for (int k = 0; k < K; ++k) r = r + get(k);
    }
  }
  uint32_t amax = __float_as_uint(r) & 0x7FFFFFFFu;
#pragma unroll
  for (int d = 16; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)amax, d, 32);
    amax = o > amax ? o : amax;
  }
  const BlockScale b = block_scale(amax);
  const uint32_t c = encode(r, b);
  if (on && i < M) {
    codes[i] = (uint8_t)c;
    if (l == 0) scales[blk] = (uint8_t)b.s;
  }
}

// ------------------------------------------------------------------------------------
// The client side
// ------------------------------------------------------------------------------------

// a + b where a NaN in a wins, quieted: the add of fedagg_flat_increment (flat_ops.hip), whose
// result does not depend on how the compiler commutes the operands.
__device__ __forceinline__ float add_in_order(float a, float b) {
#pragma clang fp contract(off)
  const float r = a + b;
  return a != a ? __uint_as_float(__float_as_uint(a) | 0x00400000u) : r;
}

// w + fl32(m * d)
__device__ __forceinline__ float increment(const float w, const float d, const float m) {
#pragma clang fp contract(off)
  const float t = m * d;
  return add_in_order(w, t);
}

// One code under the scale f, by the instruction of the vector walk.
__device__ __forceinline__ float decode_byte(const uint32_t c, const float f) {
#pragma clang fp contract(off)
  const f32x2 v = __builtin_amdgcn_cvt_pk_f32_fp8((int)c, false);
  return v[0] * f;
}

// w[0..16) += m * x[0..16), all inside one tensor: H single elements up to the 16-B alignment of w
// (a tensor's flat offset need not be a multiple of 4), then 16-B loads and stores, then the rest.
template <int H>
__device__ __forceinline__ void increment16(float* w, const float (&x)[DL_VEC], const float m) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < H; ++j) w[j] = increment(w[j], x[j], m);
  constexpr int NQ = H ? 3 : 4;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    u32x4 r = reinterpret_cast<const u32x4*>(w + H)[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = __float_as_uint(increment(__uint_as_float(r[j]), x[H + 4 * q + j], m));
    reinterpret_cast<u32x4*>(w + H)[q] = r;
  }
#pragma unroll
  for (int j = H + 4 * NQ; j < DL_VEC; ++j) w[j] = increment(w[j], x[j], m);
}

// The tensors of one launch: tensor l covers the flat elements [off[l], off[l + 1]).
struct SegArgs {
  float* p[DL_SEG];
  uint64_t off[DL_SEG + 1];
  int nl;
};

// The tensor that holds flat element e, off[0] <= e < off[nl]: the last l with off[l] <= e (an
// empty tensor is never that one).
__device__ __forceinline__ int seg_of(const SegArgs& a, const uint64_t e) {
  int lo = 0, hi = a.nl - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.off[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(DL_THREADS)
    mxdl_increment_kernel(const SegArgs a, const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales,
                          const float m, const int codes16) {
#pragma clang fp contract(off)
  const uint64_t g0 = a.off[0], g1 = a.off[a.nl];  // this launch's flat range, g1 <= M
  const uint64_t v0 = g0 / DL_VEC, nvec = (g1 + DL_VEC - 1) / DL_VEC - v0;
  for (uint64_t t = blockIdx.x; t * DL_THREADS < nvec; t += gridDim.x) {
    const uint64_t vi = t * DL_THREADS + threadIdx.x;
    if (vi >= nvec) break;
    const uint64_t i0 = (v0 + vi) * DL_VEC;  // 16 elements from a multiple of 16: one scale byte
    const float f = scale_of(scales[i0 >> 5]);
    int l = seg_of(a, i0 > g0 ? i0 : g0);
    float* w = a.p[l] + (i0 - a.off[l]);  // used only where i0 >= off[l]
    if (codes16 && i0 >= a.off[l] && i0 + DL_VEC <= a.off[l + 1]) {
      const u32x4 raw = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(codes + i0));
      float x[DL_VEC];
#pragma unroll
      for (int q = 0; q < 4; ++q) decode_dword(raw[q], f, reinterpret_cast<float(&)[4]>(x[4 * q]));
      switch ((0u - (uint32_t)(reinterpret_cast<uintptr_t>(w) >> 2)) & 3u) {  // elements up to 16-B alignment of w
        case 0: increment16<0>(w, x, m); break;
        case 1: increment16<1>(w, x, m); break;
        case 2: increment16<2>(w, x, m); break;
        default: increment16<3>(w, x, m); break;
      }
    } else {
      for (int j = 0; j < DL_VEC; ++j) {
        const uint64_t e = i0 + j;
        if (e < g0 || e >= g1) continue;  // another launch's tensor, or past the end
        while (a.off[l + 1] <= e) ++l;    // e < off[nl]: stops in range
        float* we = a.p[l] + (e - a.off[l]);
        *we = increment(*we, decode_byte(codes[e], f), m);
      }
    }
  }
}

__global__ void __launch_bounds__(DL_THREADS)
    mxdl_decode_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, const uint64_t M,
                       float* __restrict__ out, const int vec) {
#pragma clang fp contract(off)
  const uint64_t nvec = (M + DL_VEC - 1) / DL_VEC;
  for (uint64_t t = blockIdx.x; t * DL_THREADS < nvec; t += gridDim.x) {
    const uint64_t v = t * DL_THREADS + threadIdx.x;
    if (v >= nvec) break;
    const uint64_t i0 = v * DL_VEC;
    const float f = scale_of(scales[i0 >> 5]);
    if (vec && i0 + DL_VEC <= M) {
      const u32x4 raw = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(codes + i0));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float x[4];
        decode_dword(raw[q], f, x);
        u32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = __float_as_uint(x[j]);
        __builtin_nontemporal_store(r, reinterpret_cast<u32x4*>(out + i0) + q);
      }
    } else {
      for (int j = 0; j < DL_VEC && i0 + j < M; ++j) out[i0 + j] = decode_byte(codes[i0 + j], f);
    }
  }
}

unsigned grid_for(uint64_t lane_vectors) {
  uint64_t g = (lane_vectors + DL_THREADS - 1) / DL_THREADS;
  if (g < 1) g = 1;
  return (unsigned)(g > DL_GRID_CAP ? DL_GRID_CAP : g);
}

template <int KIND>
int launch_fedavg(const MxArgs& a, int K, uint64_t M, const uint64_t* h_idx, int P, uint8_t* d_out_codes,
                  uint8_t* d_out_scales, hipStream_t stream) {
  const int codes16 = (reinterpret_cast<uintptr_t>(d_out_codes) & 15u) == 0;
  const int scales16 = (reinterpret_cast<uintptr_t>(d_out_scales) & 15u) == 0;
  hipLaunchKernelGGL(mxdl_fedavg_kernel<KIND>, dim3(grid_for(2 * ((M + 31) / 32))), dim3(DL_THREADS), 0, stream, a, K,
                     M, d_out_codes, d_out_scales, codes16, scales16);
  int rc = check_launch("mxdl fedavg kernel");
  if (rc || P == 0) return rc;

  // the listed indices by block, each block once with the mask of its listed elements
  std::vector<uint64_t> idx(h_idx, h_idx + P);
  std::sort(idx.begin(), idx.end());
  PwBlocks pb;
  memset(&pb, 0, sizeof(pb));
  for (int p = 0; p <= P; ++p) {
    const bool more = p < P;
    if (more && pb.n > 0 && pb.block[pb.n - 1] == idx[p] >> 5) {
      pb.mask[pb.n - 1] |= 1u << (idx[p] & 31u);
      continue;
    }
    if (pb.n == DL_PW_BLOCKS || (!more && pb.n > 0)) {
      const unsigned grid = (unsigned)((pb.n + DL_THREADS / 32 - 1) / (DL_THREADS / 32));
      hipLaunchKernelGGL(mxdl_pairwise_kernel<KIND>, dim3(grid), dim3(DL_THREADS), 0, stream, a, pb, K, M, d_out_codes,
                         d_out_scales);
      rc = check_launch("mxdl pairwise kernel");
      if (rc) return rc;
      memset(&pb, 0, sizeof(pb));
    }
    if (more) {
      pb.block[pb.n] = idx[p] >> 5;
      pb.mask[pb.n] = 1u << (idx[p] & 31u);
      ++pb.n;
    }
  }
  return FEDAGG_OK;
}

}  // namespace

extern "C" {

int fedagg_mxdl_abi_version(void) { return FEDAGG_MXDL_ABI_VERSION; }
const char* fedagg_mxdl_last_error(void) { return fedagg_lib_error::g_error; }

int fedagg_mxdl_blocking(int* tile_elems, int* lane_elems, int* k_group) {
  if (tile_elems) *tile_elems = DL_TILE;
  if (lane_elems) *lane_elems = DL_VEC;
  if (k_group) *k_group = DL_U;
  return FEDAGG_OK;
}

int fedagg_mxdl_fedavg(int in_kind, const uint8_t* const* d_codes, const uint8_t* const* d_scales, const float* h_w,
                       int K, uint64_t M, const uint64_t* h_idx, int P, uint8_t* d_out_codes, uint8_t* d_out_scales,
                       void* stream) {
  if (in_kind != E4M3 && in_kind != E2M1)
    return fail(FEDAGG_EINVAL, "mxdl fedavg: in_kind %lld is not FEDAGG_MXDL_E4M3 / FEDAGG_MXDL_E2M1", (long long)in_kind);
  if (K <= 0) return fail(FEDAGG_EINVAL, "mxdl fedavg: K must be positive (K=%lld)", (long long)K);
  if (K > FEDAGG_MXDL_KMAX)
    return fail(FEDAGG_EINVAL, "mxdl fedavg: at most FEDAGG_MXDL_KMAX clients per call, a continued accumulator "
                               "needs the fp32 row (K=%lld)", (long long)K);
  if (!d_codes) return fail(FEDAGG_EINVAL, "mxdl fedavg: d_codes is NULL");
  if (!d_scales) return fail(FEDAGG_EINVAL, "mxdl fedavg: d_scales is NULL");
  if (!h_w) return fail(FEDAGG_EINVAL, "mxdl fedavg: h_w is NULL");
  if (P < 0) return fail(FEDAGG_EINVAL, "mxdl fedavg: P is negative (P=%lld)", (long long)P);
  if (P > 0 && !h_idx) return fail(FEDAGG_EINVAL, "mxdl fedavg: h_idx is NULL with P > 0");
  if (M == 0) return FEDAGG_OK;
  if (M > (1ull << 44)) return fail(FEDAGG_EINVAL, "mxdl fedavg: M is too large");
  MxArgs a;
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < K; ++k) {
    if (!d_codes[k]) return fail(FEDAGG_EINVAL, "mxdl fedavg: code row %lld is NULL", (long long)k);
    if (reinterpret_cast<uintptr_t>(d_codes[k]) & 15u)
      return fail(FEDAGG_EINVAL, "mxdl fedavg: code row %lld is not 16-B aligned", (long long)k);
    if (!d_scales[k]) return fail(FEDAGG_EINVAL, "mxdl fedavg: scale row %lld is NULL", (long long)k);
    a.c[k] = d_codes[k];
    a.s[k] = d_scales[k];
    a.w[k] = h_w[k];
  }
  if (!d_out_codes) return fail(FEDAGG_EINVAL, "mxdl fedavg: d_out_codes is NULL");
  if (!d_out_scales) return fail(FEDAGG_EINVAL, "mxdl fedavg: d_out_scales is NULL");
  for (int p = 0; p < P; ++p)
    if (h_idx[p] >= M) return fail(FEDAGG_EINVAL, "mxdl fedavg: numel == 1 index %lld is out of range", (long long)p);
  if (in_kind == E4M3) return launch_fedavg<E4M3>(a, K, M, h_idx, P, d_out_codes, d_out_scales, (hipStream_t)stream);
  return launch_fedavg<E2M1>(a, K, M, h_idx, P, d_out_codes, d_out_scales, (hipStream_t)stream);
}

int fedagg_mxdl_increment(float* const* d_layers, const uint64_t* numel, int L, const uint8_t* d_codes,
                          const uint8_t* d_scales, uint64_t M, double multiplier, void* stream) {
  if (L < 0) return fail(FEDAGG_EINVAL, "mxdl increment: L is negative (L=%lld)", (long long)L);
  if (L > 0 && !d_layers) return fail(FEDAGG_EINVAL, "mxdl increment: d_layers is NULL");
  if (L > 0 && !numel) return fail(FEDAGG_EINVAL, "mxdl increment: numel is NULL");
  if (M > (1ull << 44)) return fail(FEDAGG_EINVAL, "mxdl increment: M is too large");
  uint64_t total = 0;
  for (int l = 0; l < L; ++l) {
    if (numel[l] > (1ull << 44)) return fail(FEDAGG_EINVAL, "mxdl increment: tensor %lld is too large", (long long)l);
    if (!d_layers[l] && numel[l]) return fail(FEDAGG_EINVAL, "mxdl increment: tensor %lld is NULL", (long long)l);
    if (reinterpret_cast<uintptr_t>(d_layers[l]) & 3u)
      return fail(FEDAGG_EINVAL, "mxdl increment: tensor %lld is not 4-B aligned", (long long)l);
    total += numel[l];
  }
  if (total != M)
    return fail(FEDAGG_EINVAL, "mxdl increment: the tensors hold %llu elements, the update %llu",
                (unsigned long long)total, (unsigned long long)M);
  if (M == 0) return FEDAGG_OK;
  if (!d_codes) return fail(FEDAGG_EINVAL, "mxdl increment: d_codes is NULL");
  if (!d_scales) return fail(FEDAGG_EINVAL, "mxdl increment: d_scales is NULL");

  const int codes16 = (reinterpret_cast<uintptr_t>(d_codes) & 15u) == 0;
  uint64_t off = 0;
  for (int l0 = 0; l0 < L; l0 += DL_SEG) {
    SegArgs a;
    memset(&a, 0, sizeof(a));
    a.nl = L - l0 < DL_SEG ? L - l0 : DL_SEG;
    for (int l = 0; l < a.nl; ++l) {
      a.p[l] = d_layers[l0 + l];
      a.off[l] = off;
      off += numel[l0 + l];
    }
    a.off[a.nl] = off;
    if (a.off[a.nl] == a.off[0]) continue;
    const uint64_t nvec = (a.off[a.nl] + DL_VEC - 1) / DL_VEC - a.off[0] / DL_VEC;
    hipLaunchKernelGGL(mxdl_increment_kernel, dim3(grid_for(nvec)), dim3(DL_THREADS), 0, (hipStream_t)stream, a,
                       d_codes, d_scales, (float)multiplier, codes16);
    const int rc = check_launch("mxdl increment kernel");
    if (rc) return rc;
  }
  return FEDAGG_OK;
}

int fedagg_mxdl_decode(const uint8_t* d_codes, const uint8_t* d_scales, uint64_t M, float* d_out, void* stream) {
  if (M == 0) return FEDAGG_OK;
  if (M > (1ull << 44)) return fail(FEDAGG_EINVAL, "mxdl decode: M is too large");
  if (!d_codes) return fail(FEDAGG_EINVAL, "mxdl decode: d_codes is NULL");
  if (!d_scales) return fail(FEDAGG_EINVAL, "mxdl decode: d_scales is NULL");
  if (!d_out) return fail(FEDAGG_EINVAL, "mxdl decode: d_out is NULL");
  if (reinterpret_cast<uintptr_t>(d_out) & 3u) return fail(FEDAGG_EINVAL, "mxdl decode: d_out is not 4-B aligned");
  const int vec = ((reinterpret_cast<uintptr_t>(d_codes) | reinterpret_cast<uintptr_t>(d_out)) & 15u) == 0;
  hipLaunchKernelGGL(mxdl_decode_kernel, dim3(grid_for((M + DL_VEC - 1) / DL_VEC)), dim3(DL_THREADS), 0,
                     (hipStream_t)stream, d_codes, d_scales, M, d_out, vec);
  return check_launch("mxdl decode kernel");
}

}  // extern "C"
