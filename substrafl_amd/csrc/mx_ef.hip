// mx_ef.hip -- libfedagg_mxef.so (include/fedagg_mxef.h): the MXFP8 quantiser with error
// feedback, fused.  One pass reads the update x and the fp32 residual once and writes the codes,
// the scale bytes and the new residual once: 13.03 bytes per element for fp32 updates, 11.03 for
// bf16, where add + quantise + decode + subtract from separate kernels would move 29.
//
// Arithmetic per element (fp32, never contracted: -ffp-contract=off and the pragma in every body):
//   r = fl32(x + res);  (code, s) = the encode rule of fedagg_mx.h on r;  d = decode(code, s)
//   res' = fl32(r - d) where the block is finite and d is finite, +0.0 otherwise
//
// The vector walk.  A lane owns MXEF_LANE = 8 consecutive elements, so the 4 lanes of a quad own
// one scale block, a wave 512 contiguous elements and a workgroup step MXEF_TILE = 2048.
//   loads   x in 16-B non-temporal loads (two per lane for fp32, one for bf16), res in two
//   maximum the in-lane maximum of the 8 magnitude bit patterns, then two DPP quad permutes (lane
//           xor 1, lane xor 2): no LDS, no atomics; NaN and Inf sort above every finite value
//   encode  the integer path of mx_codec.h (e4m3_of), the bits of mx.hip's quantiser
//   decode  v_cvt_pk_f32_fp8 on the packed codes times the scale, as mx.hip's decode_vec
//   stores  the 8 codes of a lane as one 8-B store (512 contiguous bytes per wave), res' as two
//           16-B stores; the wave's 16 scale bytes are collected through 16 bytes of LDS into lane
//           0 and leave as ONE 16-B store when the scale row is 16-B aligned and the wave is whole,
//           as byte stores from the quads' first lanes otherwise.  Plain vector-unit stores only.
// A non-finite or all-zero block takes the same instructions: its maximum is replaced by 1.0 for
// the scale computation and s, the codes and res' are selected at the end (no divergent branch).
// The grid is capped at MXEF_GRID workgroups (8 per CU of an MI355X: at 64 VGPRs or fewer all of
// them are resident at once), each walking tiles blockIdx.x, blockIdx.x + gridDim.x, ...
//
// The element walk.  One element per lane, the 32 lanes of a half-wave one scale block, the shape
// of mx.hip's quantiser with the residual added: the last M % 32 elements, and the whole call when
// d_x or d_res is not 16-B aligned or d_codes not 8-B aligned.  Same helpers, same decode
// instruction, so the two walks give identical bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "fedagg_mxef.h"
#include "lib_error.h"
#include "mx_codec.h"

#define MXEF_THREADS 256                       // threads per workgroup
#define MXEF_LANE 8                            // elements per lane of the vector walk (lane_elems)
#define MXEF_TILE (MXEF_THREADS * MXEF_LANE)   // elements per workgroup step (tile_elems)
#define MXEF_GRID 2048u                        // workgroups at most

namespace {

using fedagg_internal::block_scale;
using fedagg_internal::BlockScale;
using fedagg_internal::encode;
using fedagg_lib_error::fail;
constexpr auto check_launch = fedagg_lib_error::check_launch<FEDAGG_OK, FEDAGG_EHIP>;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// The maximum over the 4 lanes of a quad: quad_perm [1,0,3,2] is lane xor 1, [2,3,0,1] lane xor 2.
__device__ __forceinline__ uint32_t quad_max(uint32_t a) {
  uint32_t o = (uint32_t)__builtin_amdgcn_mov_dpp((int)a, 0xB1, 0xF, 0xF, true);
  a = o > a ? o : a;
  o = (uint32_t)__builtin_amdgcn_mov_dpp((int)a, 0x4E, 0xF, 0xF, true);
  return o > a ? o : a;
}

// res' from r and the hardware's decode v of its code.
__device__ __forceinline__ float residual(const float r, const float v, const BlockScale& b) {
#pragma clang fp contract(off)
  const float d = v * b.f;
  const bool fin = (__float_as_uint(d) & 0x7FFFFFFFu) < 0x7F800000u;
  const float e = r - d;
  return (fin && !b.bad) ? e : 0.0f;
}

template <int KIND>
__device__ __forceinline__ void load_x8(const void* __restrict__ x_, const uint64_t i, float (&x)[MXEF_LANE]) {
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
// elements from mv on go one per lane.  scales16: the scale row is 16-B aligned.
template <int KIND>
__global__ void __launch_bounds__(MXEF_THREADS)
    mxef_quantize_kernel(const void* __restrict__ x_, const uint64_t mv, const uint64_t M, float* __restrict__ res,
                         uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, const int scales16) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) uint8_t sc_stage[MXEF_THREADS / 64][16];
  const int lane = threadIdx.x & 63;
  uint8_t* sc_wave = sc_stage[threadIdx.x / 64];

  for (uint64_t t = blockIdx.x; t * MXEF_TILE < mv; t += gridDim.x) {
    const uint64_t i = t * MXEF_TILE + (uint64_t)threadIdx.x * MXEF_LANE;  // this lane's first element
    const uint64_t wave_i = i - (uint64_t)lane * MXEF_LANE;
    const bool wave_whole = wave_i + 64 * MXEF_LANE <= mv;  // wave-uniform
    if (i < mv) {  // mv is a multiple of 32: the 4 lanes of a quad are in range together
      float r[MXEF_LANE];
      load_x8<KIND>(x_, i, r);
      u32x4* rp = reinterpret_cast<u32x4*>(res + i);
      uint32_t a = 0;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const u32x4 v = __builtin_nontemporal_load(rp + q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          r[4 * q + j] = r[4 * q + j] + __uint_as_float(v[j]);
          const uint32_t mag = __float_as_uint(r[4 * q + j]) & 0x7FFFFFFFu;
          a = mag > a ? mag : a;
        }
      }
      const BlockScale b = block_scale(quad_max(a));
      u32x2 c;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) w |= encode(r[4 * q + j], b) << (8 * j);
        c[q] = w;
      }
      __builtin_nontemporal_store(c, reinterpret_cast<u32x2*>(codes + i));
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[q], false);  // bytes 0, 1
        const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[q], true);   // bytes 2, 3
        u32x4 o;
        o[0] = __float_as_uint(residual(r[4 * q + 0], lo[0], b));
        o[1] = __float_as_uint(residual(r[4 * q + 1], lo[1], b));
        o[2] = __float_as_uint(residual(r[4 * q + 2], hi[0], b));
        o[3] = __float_as_uint(residual(r[4 * q + 3], hi[1], b));
        __builtin_nontemporal_store(o, rp + q);
      }
      if (!(wave_whole && scales16)) {
        if ((lane & 3) == 0) scales[i >> 5] = (uint8_t)b.s;
      } else if ((lane & 3) == 0) {
        sc_wave[lane >> 2] = (uint8_t)b.s;
      }
    }
    if (wave_whole && scales16) {  // all 64 lanes are here
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (lane == 0) *reinterpret_cast<u32x4*>(scales + (wave_i >> 5)) = *reinterpret_cast<const u32x4*>(sc_wave);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // WAR before the next step's bytes
      __builtin_amdgcn_wave_barrier();
    }
  }

  // one element per lane from mv on; every lane of a block walks the same steps
  const uint64_t padded = (M + 31) & ~(uint64_t)31;
  const uint64_t stride = (uint64_t)gridDim.x * MXEF_THREADS;
  for (uint64_t i = mv + (uint64_t)blockIdx.x * MXEF_THREADS + threadIdx.x; i < padded; i += stride) {
    float r = 0.0f;  // lanes past M hold +0: no effect on the maximum
    if (i < M) {
      float x;
      if constexpr (KIND == FEDAGG_BF16) x = __uint_as_float((uint32_t)static_cast<const uint16_t*>(x_)[i] << 16);
      else x = static_cast<const float*>(x_)[i];
      r = x + res[i];
    }
    uint32_t a = __float_as_uint(r) & 0x7FFFFFFFu;
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)a, d, 32);
      a = o > a ? o : a;
    }
    const BlockScale b = block_scale(a);
    const uint32_t c = encode(r, b);
    const f32x2 v = __builtin_amdgcn_cvt_pk_f32_fp8((int)c, false);
    if (i < M) {
      codes[i] = (uint8_t)c;
      res[i] = residual(r, v[0], b);
      if ((i & 31) == 0) scales[i >> 5] = (uint8_t)b.s;
    }
  }
}

bool overlap(const void* p, uint64_t np, const void* q, uint64_t nq) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + nq && b < a + np;
}

}  // namespace

extern "C" {

int fedagg_mxef_abi_version(void) { return FEDAGG_MXEF_ABI_VERSION; }
const char* fedagg_mxef_last_error(void) { return fedagg_lib_error::g_error; }

int fedagg_mxef_blocking(int* lane_elems, int* tile_elems, uint64_t* second_step_elems) {
  if (lane_elems) *lane_elems = MXEF_LANE;
  if (tile_elems) *tile_elems = MXEF_TILE;
  if (second_step_elems) *second_step_elems = (uint64_t)MXEF_GRID * MXEF_TILE;
  return FEDAGG_OK;
}

int fedagg_mxef_quantize(const void* d_x, int kind, uint64_t M, float* d_res, uint8_t* d_codes, uint8_t* d_scales,
                         void* stream) {
  if (kind != FEDAGG_F32 && kind != FEDAGG_BF16)
    return fail(FEDAGG_EINVAL, "mxef quantize: kind %lld is not FEDAGG_F32 / FEDAGG_BF16", (long long)kind);
  if (M == 0) return FEDAGG_OK;
  if (M > (1ull << 44)) return fail(FEDAGG_EINVAL, "mxef quantize: M is too large");
  const uint64_t esz = kind == FEDAGG_F32 ? 4 : 2;
  if (!d_x) return fail(FEDAGG_EINVAL, "mxef quantize: d_x is NULL");
  if (reinterpret_cast<uintptr_t>(d_x) & (esz - 1))
    return fail(FEDAGG_EINVAL, "mxef quantize: d_x is not aligned to its element size");
  if (!d_res) return fail(FEDAGG_EINVAL, "mxef quantize: d_res is NULL");
  if (reinterpret_cast<uintptr_t>(d_res) & 3u) return fail(FEDAGG_EINVAL, "mxef quantize: d_res is not 4-B aligned");
  if (!d_codes) return fail(FEDAGG_EINVAL, "mxef quantize: d_codes is NULL");
  if (!d_scales) return fail(FEDAGG_EINVAL, "mxef quantize: d_scales is NULL");
  const uint64_t nb = (M + 31) / 32;
  if (overlap(d_res, 4 * M, d_x, esz * M)) return fail(FEDAGG_EINVAL, "mxef quantize: d_res overlaps d_x");
  if (overlap(d_res, 4 * M, d_codes, M)) return fail(FEDAGG_EINVAL, "mxef quantize: d_res overlaps d_codes");
  if (overlap(d_res, 4 * M, d_scales, nb)) return fail(FEDAGG_EINVAL, "mxef quantize: d_res overlaps d_scales");

  const bool vec = !((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_res)) & 15u) &&
                   !(reinterpret_cast<uintptr_t>(d_codes) & 7u);
  const uint64_t mv = vec ? M & ~(uint64_t)31 : 0;
  const int scales16 = (reinterpret_cast<uintptr_t>(d_scales) & 15u) == 0;
  const uint64_t steps_v = (mv + MXEF_TILE - 1) / MXEF_TILE, steps_e = (M - mv + MXEF_THREADS - 1) / MXEF_THREADS;
  uint64_t g = steps_v > steps_e ? steps_v : steps_e;
  if (g > MXEF_GRID) g = MXEF_GRID;
  if (kind == FEDAGG_F32)
    hipLaunchKernelGGL(mxef_quantize_kernel<FEDAGG_F32>, dim3((unsigned)g), dim3(MXEF_THREADS), 0, (hipStream_t)stream,
                       d_x, mv, M, d_res, d_codes, d_scales, scales16);
  else
    hipLaunchKernelGGL(mxef_quantize_kernel<FEDAGG_BF16>, dim3((unsigned)g), dim3(MXEF_THREADS), 0, (hipStream_t)stream,
                       d_x, mv, M, d_res, d_codes, d_scales, scales16);
  return check_launch("mxef quantize kernel");
}

}  // extern "C"
