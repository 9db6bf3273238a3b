// mx_codec.h -- the MXFP8 element codec as device code (the rules of include/fedagg_mx.h), shared
// by mx.hip (libfedagg_mx.so), mx_ef.hip (libfedagg_mxef.so) and mx_down.hip (libfedagg_mxdl.so).
// Every helper carries `#pragma clang fp contract(off)`; the files are compiled with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fedagg_internal {

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

// The scale byte s = e + 127 of a block whose maximum magnitude has the bits a (finite, not zero),
// and inv = 2^-e, the factor its elements are multiplied by before rounding to e4m3fn.
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
  int e = fl - 8;
  if (mant > 0x00E80000u) e += 1;  // amax * 2^-e > 464 = 1.8125 * 2^8
  e = e < -127 ? -127 : (e > 127 ? 127 : e);
  const uint32_t f = (uint32_t)(127 - e);                      // exponent field of 2^-e
  inv = __uint_as_float(f ? f << 23 : 0x00400000u);            // 2^-127 is a subnormal
  return (uint32_t)(e + 127);
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

// The code of r under the block's scale (a bad block's codes are 0x00; a zero block's carry the signs:
// +-0 * inv is +-0 and e4m3_of(0) is 0).
__device__ __forceinline__ uint32_t encode(const float r, const BlockScale& b) {
#pragma clang fp contract(off)
  const float y = r * b.inv;
  const uint32_t yu = __float_as_uint(y);
  const uint32_t c = e4m3_of(yu & 0x7FFFFFFFu) | ((yu >> 24) & 0x80u);
  return b.bad ? 0u : c;
}

}  // namespace fedagg_internal
