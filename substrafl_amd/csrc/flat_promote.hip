// flat_promote.hip -- libfedagg_promote.so (include/fedagg_promote.h): the client flat ops of a
// 16-bit model next to fp64 operands, i.e. torch's type promotion in weight_manager's per-layer
// loops (weight_manager.py:103-137, 182-212) done as one launch over up to SEG_GROUP layers.
// Geometry as in flat_ops.hip: workgroup b serves layer l with block_start[l] <= b <
// block_start[l+1], elements [(b - block_start[l]) * SEG_CHUNK, ...).
// Bit parity with torch needs every product, sum and conversion rounded on its own: the file is
// compiled with -ffp-contract=off AND every kernel body and per-element helper carries
// `#pragma clang fp contract(off)`; the double -> float -> 16-bit conversion of the increment is
// kept as two roundings by the register barriers of round_to.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "fedagg_promote.h"

#define PR_BLOCK 256    // threads per workgroup
#define SEG_GROUP 32    // layers per launch
#define SEG_CHUNK 8192  // elements per workgroup
#define PR_W 8          // elements per lane and step of the wide path: 16 B of a 16-bit operand

namespace {

thread_local char g_error[256] = "";
std::atomic<int> g_vec{1};  // the "vec" knob

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

struct PromoteArgs {
  const void* p[FEDAGG_FLAT_MAX_LISTS][SEG_GROUP];  // list-major layer pointers
  uint64_t n[SEG_GROUP];
  uint64_t flat_off[SEG_GROUP];
  uint32_t block_start[SEG_GROUP + 1];
  double coeff[FEDAGG_FLAT_MAX_LISTS];
  uint32_t f64;  // bit j says list j is fp64 (uniform per launch: the branches on it are scalar)
  int vec;       // the "vec" knob
  int nl, nlists;
};

__device__ __forceinline__ int seg_of_block(const PromoteArgs& a, uint32_t b) {
  int l = 0;
  while (l + 1 < a.nl && a.block_start[l + 1] <= b) ++l;  // scalar, <= SEG_GROUP steps
  return l;
}

// 16-bit elements are handled as their bit patterns; widen<K> is exact, round_to<K> is torch's
// rounding of an fp32 value to K (nearest even, overflow to +-inf, NaN stays NaN).
template <int K>
__device__ __forceinline__ float widen(uint16_t b) {
  if constexpr (K == FEDAGG_F16) return (float)__builtin_bit_cast(_Float16, b);
  else return __uint_as_float((uint32_t)b << 16);
}

template <int K>
__device__ __forceinline__ uint16_t round_to(float f) {
  if constexpr (K == FEDAGG_F16) {
    // The fp32 value and the converted bits each pass through a register of their own, so the
    // rounding is one plain v_cvt_f16_f32 of the fp32 value: the compiler neither folds the
    // operation before it (a multiply, or the double -> float conversion of the increment) into
    // the conversion nor pairs two conversions into a packed one.
    asm("" : "+v"(f));
    uint32_t r = __builtin_bit_cast(uint16_t, (_Float16)f);
    asm("" : "+v"(r));
    return (uint16_t)r;
  } else {
    asm("" : "+v"(f));  // bf16: the bits of the fp32 value as it was rounded from the double
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  }
}

// a + b where a NaN in a wins (flat_ops.hip add_in_order): the compiler commutes a plain a + b as
// it likes, differently in the wide loop and in the tail, and the hardware returns the payload of
// the first NaN source.  Spelled out, a result does not depend on which loop made it.
__device__ __forceinline__ float add_in_order(float a, float b) {
#pragma clang fp contract(off)
  const float r = a + b;
  return a != a ? __uint_as_float(__float_as_uint(a) | 0x00400000u) : r;  // a, quieted
}
__device__ __forceinline__ double add_in_order(double a, double b) {
#pragma clang fp contract(off)
  const double r = a + b;
  return a != a ? __longlong_as_double(__double_as_longlong(a) | 0x0008000000000000ll) : r;
}

// x * c for a 16-bit list.  The rule (torch on the CPU, and torch's vectorised kernels on the
// device): the fp32 product, rounded once more to T.  torch on ROCm (2.10) serves a contiguous
// 16-B aligned fp16 tensor in blocks of TORCH_F16_BLOCK elements and hands the tensor's remainder
// (numel mod 2048 trailing elements; a whole tensor smaller than a block) to an unrolled loop
// whose multiply and conversion are one fused operation: the EXACT product is rounded once to
// fp16, and an exact zero product is +0 whatever the signs (a fused multiply-add onto +0).
// `once` says the element lies in that remainder of its layer; the reference's layers are whole
// aligned tensors.  bf16 tensors take the rule everywhere (measured: no element differs).
#define TORCH_F16_BLOCK 2048
static_assert(SEG_CHUNK % TORCH_F16_BLOCK == 0 && TORCH_F16_BLOCK % PR_W == 0,
              "a lane's 8 elements lie inside one torch block or in the remainder");
template <int K>
__device__ __forceinline__ uint16_t product16(uint16_t x, float c, bool once) {
#pragma clang fp contract(off)
  const float xf = widen<K>(x);
  float p = xf * c;
  if constexpr (K == FEDAGG_F16) {
    if (once) {
      // one rounding of the exact product: p goes to fp16 through round-to-odd.  e is the exact
      // error of p (an explicit fma); where it is not zero the exact product lies strictly
      // between two floats, and the one of them with an odd last bit rounds to fp16 as the
      // exact product does (24 bits are more than fp16's 11 + 2).
      const float e = __builtin_fmaf(xf, c, -p);
      uint32_t pu = __float_as_uint(p);
      if (e != 0.0f && e == e && (pu & 0x7f800000u) != 0x7f800000u && (pu & 0x7fffffffu) != 0u) {
        const bool beyond = (e > 0.0f) == (p > 0.0f);  // the exact product is larger in magnitude than p
        pu = (beyond ? pu : pu - 1u) | 1u;
        p = __uint_as_float(pu);
      }
      const uint16_t h = round_to<K>(p);
      return (h == 0x8000u && (xf == 0.0f || c == 0.0f)) ? (uint16_t)0 : h;
    }
  }
  return round_to<K>(p);
}

// One step of Python's sum() over x_j * c_j for one element; the wide loop and the tail both call
// it.  The running sum is (ah, T) until the first fp64 operand and (ad, fp64) from there on;
// acc64 / is64 / first are uniform over the launch.  Of (xh, xd) the one of the list's kind is read.
template <int K>
__device__ __forceinline__ void wsum_step(bool first, bool acc64, bool is64, uint16_t& ah, double& ad, uint16_t xh,
                                          double xd, float cf, double cd, bool once) {
#pragma clang fp contract(off)
  if (is64) {
    const double p = xd * cd;  // fp64 tensor * Python scalar: in fp64
    if (first) ad = add_in_order(0.0, p);  // int 0 + p_0: -0 becomes +0
    else ad = add_in_order(acc64 ? ad : (double)widen<K>(ah), p);
  } else {
    const uint16_t p = product16<K>(xh, cf, once);  // the scalar rounded to fp32
    if (first) ah = round_to<K>(add_in_order(0.0f, widen<K>(p)));
    else if (acc64) ad = add_in_order(ad, (double)widen<K>(p));
    else ah = round_to<K>(add_in_order(widen<K>(ah), widen<K>(p)));
  }
}

// w + m * u, w of kind K and u fp64: the product and the sum in fp64, the result to K through float
template <int K>
__device__ __forceinline__ uint16_t increment(uint16_t w, double u, double m) {
#pragma clang fp contract(off)
  const double t = m * u;
  const double s = add_in_order((double)widen<K>(w), t);
  return round_to<K>((float)s);
}

// 8 elements of a 16-bit layer as one 16-B access; 2 doubles as one 16-B access declared at the
// 8-B alignment a slice of the bucket (or an fp64 layer) really has.
typedef uint16_t Half8 __attribute__((ext_vector_type(8), aligned(16)));
typedef double Double2 __attribute__((ext_vector_type(2), aligned(8)));

__device__ __forceinline__ void load8(const double* p, double (&x)[PR_W]) {
#pragma unroll
  for (int q = 0; q < PR_W / 2; ++q) {
    const Double2 v = reinterpret_cast<const Double2*>(p)[q];
    x[2 * q] = v[0];
    x[2 * q + 1] = v[1];
  }
}
__device__ __forceinline__ void store8(double* p, const double (&x)[PR_W]) {
#pragma unroll
  for (int q = 0; q < PR_W / 2; ++q) {
    Double2 v;
    v[0] = x[2 * q];
    v[1] = x[2 * q + 1];
    reinterpret_cast<Double2*>(p)[q] = v;
  }
}

// Are the layer's 16-bit pointers all 16-B aligned?  (fp64 operands only need their 8 B.)
__device__ __forceinline__ bool wide_layer(const PromoteArgs& a, int l) {
  uintptr_t bits = 0;
  for (int j = 0; j < a.nlists; ++j)
    if (!((a.f64 >> j) & 1u)) bits |= reinterpret_cast<uintptr_t>(a.p[j][l]);
  return a.vec && (bits & 15u) == 0;
}

template <int K>
__global__ void __launch_bounds__(PR_BLOCK) promote_wsum_kernel(const PromoteArgs a, double* __restrict__ flat) {
#pragma clang fp contract(off)
  const int l = seg_of_block(a, blockIdx.x);
  const uint64_t base = (uint64_t)(blockIdx.x - a.block_start[l]) * SEG_CHUNK;
  const uint64_t n = a.n[l];
  const uint64_t end = base + SEG_CHUNK < n ? base + SEG_CHUNK : n;
  double* f = flat + a.flat_off[l];
  float cf[FEDAGG_FLAT_MAX_LISTS];
#pragma unroll
  for (int j = 0; j < FEDAGG_FLAT_MAX_LISTS; ++j) cf[j] = (float)a.coeff[j];  // torch rounds the scalar
  const uint64_t nfull = n & ~(uint64_t)(TORCH_F16_BLOCK - 1);  // from here on: the remainder of the layer as a torch tensor
  uint64_t tail = base + threadIdx.x;  // where the element-by-element loop starts
  if (wide_layer(a, l)) {
    const uint64_t vend = base + ((end - base) & ~(uint64_t)(PR_W - 1));
    for (uint64_t i = base + PR_W * (uint64_t)threadIdx.x; i < vend; i += PR_W * (uint64_t)PR_BLOCK) {
      const bool once = i >= nfull;
      uint16_t ah[PR_W] = {};
      double ad[PR_W] = {};
      bool acc64 = false;
      for (int j = 0; j < a.nlists; ++j) {
        const bool is64 = (a.f64 >> j) & 1u;
        Half8 xh = 0;
        double xd[PR_W] = {};
        if (is64) load8(static_cast<const double*>(a.p[j][l]) + i, xd);
        else xh = *reinterpret_cast<const Half8*>(static_cast<const uint16_t*>(a.p[j][l]) + i);
#pragma unroll
        for (int e = 0; e < PR_W; ++e) wsum_step<K>(j == 0, acc64, is64, ah[e], ad[e], xh[e], xd[e], cf[j], a.coeff[j], once);
        acc64 = acc64 || is64;
      }
      store8(f + i, ad);  // the launcher sends no call without an fp64 list: the sum is fp64 by now
    }
    tail = vend + threadIdx.x;
  }
  for (uint64_t i = tail; i < end; i += PR_BLOCK) {
    uint16_t ah = 0;
    double ad = 0.0;
    bool acc64 = false;
    for (int j = 0; j < a.nlists; ++j) {
      const bool is64 = (a.f64 >> j) & 1u;
      const uint16_t xh = is64 ? (uint16_t)0 : static_cast<const uint16_t*>(a.p[j][l])[i];
      const double xd = is64 ? static_cast<const double*>(a.p[j][l])[i] : 0.0;
      wsum_step<K>(j == 0, acc64, is64, ah, ad, xh, xd, cf[j], a.coeff[j], i >= nfull);
      acc64 = acc64 || is64;
    }
    f[i] = ad;
  }
}

template <int K>
__global__ void __launch_bounds__(PR_BLOCK) promote_increment_kernel(const PromoteArgs a, double* __restrict__ flat) {
#pragma clang fp contract(off)
  const int l = seg_of_block(a, blockIdx.x);
  const uint64_t base = (uint64_t)(blockIdx.x - a.block_start[l]) * SEG_CHUNK;
  const uint64_t n = a.n[l];
  const uint64_t end = base + SEG_CHUNK < n ? base + SEG_CHUNK : n;
  const double* f = flat + a.flat_off[l];  // only read
  uint16_t* w = const_cast<uint16_t*>(static_cast<const uint16_t*>(a.p[0][l]));
  const double m = a.coeff[0];
  uint64_t tail = base + threadIdx.x;
  if (wide_layer(a, l)) {
    const uint64_t vend = base + ((end - base) & ~(uint64_t)(PR_W - 1));
    for (uint64_t i = base + PR_W * (uint64_t)threadIdx.x; i < vend; i += PR_W * (uint64_t)PR_BLOCK) {
      Half8 v = *reinterpret_cast<const Half8*>(w + i);
      double u[PR_W];
      load8(f + i, u);
#pragma unroll
      for (int e = 0; e < PR_W; ++e) v[e] = increment<K>(v[e], u[e], m);
      *reinterpret_cast<Half8*>(w + i) = v;
    }
    tail = vend + threadIdx.x;
  }
  for (uint64_t i = tail; i < end; i += PR_BLOCK) w[i] = increment<K>(w[i], f[i], m);
}

// ------------------------------------------------------------------------------------
// Launch: every argument is checked over all layers first, then the groups are launched.
// ------------------------------------------------------------------------------------
bool is_16bit_kind(int k) { return k == FEDAGG_F16 || k == FEDAGG_BF16; }

using Kernel = void (*)(const PromoteArgs, double*);

// ptrs is list-major [nlists][L]; f64 bit j: list j is fp64, else 16-bit
int promote_launch(Kernel kernel, const void* const* ptrs, uint32_t f64, int nlists,
                   const double* coeffs, const uint64_t* numel, int L, const double* flat, void* stream) {
  if (L < 0) return fail(FEDAGG_EINVAL, "promote op: L is negative (L=%lld)", L);
  if (L > 0 && !ptrs) return fail(FEDAGG_EINVAL, "promote op: d_layers is NULL");
  if (L > 0 && !numel) return fail(FEDAGG_EINVAL, "promote op: numel is NULL");
  uint64_t total = 0;
  for (int l = 0; l < L; ++l) {
    for (int j = 0; j < nlists; ++j) {
      const uintptr_t p = reinterpret_cast<uintptr_t>(ptrs[(size_t)j * L + l]);
      const bool is64 = (f64 >> j) & 1u;
      if (!p && numel[l]) return fail(FEDAGG_EINVAL, "promote op: NULL layer pointer %lld", l);
      if (is64 && (p & 7u)) return fail(FEDAGG_EINVAL, "promote op: fp64 layer pointer %lld is not 8-B aligned", l);
      if (!is64 && (p & 1u)) return fail(FEDAGG_EINVAL, "promote op: 16-bit layer pointer %lld is not 2-B aligned", l);
    }
    if (numel[l] > (1ull << 44)) return fail(FEDAGG_EINVAL, "promote op: layer %lld is too large", l);
    total += numel[l];
  }
  if (total && !flat) return fail(FEDAGG_EINVAL, "promote op: the fp64 bucket d_flat is NULL");
  if (reinterpret_cast<uintptr_t>(flat) & 7u) return fail(FEDAGG_EINVAL, "promote op: the fp64 bucket d_flat is not 8-B aligned");

  uint64_t off = 0;
  for (int l0 = 0; l0 < L; l0 += SEG_GROUP) {
    const int nl = (L - l0) < SEG_GROUP ? (L - l0) : SEG_GROUP;
    PromoteArgs a;
    memset(&a, 0, sizeof(a));
    a.nl = nl;
    a.nlists = nlists;
    a.f64 = f64;
    a.vec = g_vec.load(std::memory_order_relaxed);
    for (int j = 0; j < nlists; ++j) a.coeff[j] = coeffs ? coeffs[j] : 1.0;
    uint64_t blocks = 0;
    for (int l = 0; l < nl; ++l) {
      for (int j = 0; j < nlists; ++j) a.p[j][l] = ptrs[(size_t)j * L + l0 + l];
      a.n[l] = numel[l0 + l];
      a.flat_off[l] = off;
      a.block_start[l] = (uint32_t)blocks;
      off += numel[l0 + l];
      blocks += (numel[l0 + l] + SEG_CHUNK - 1) / SEG_CHUNK;
    }
    a.block_start[nl] = (uint32_t)blocks;
    if (blocks == 0) continue;
    if (blocks > 0x7fffffffull) return fail(FEDAGG_EINVAL, "promote op: too many elements in one launch group (layer %lld on)", l0);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(PR_BLOCK), 0, (hipStream_t)stream, a,
                       const_cast<double*>(flat));
    const int rc = check_launch("promote op kernel");
    if (rc) return rc;
  }
  return FEDAGG_OK;
}

}  // namespace

extern "C" {

int fedagg_promote_abi_version(void) { return FEDAGG_PROMOTE_ABI_VERSION; }
const char* fedagg_promote_last_error(void) { return g_error; }

int fedagg_promote_tune(const char* key, int value) {
  if (!key || strcmp(key, "vec") != 0) return fail(FEDAGG_EINVAL, "promote tune: unknown key");
  if (value != 0 && value != 1) return fail(FEDAGG_EINVAL, "promote tune: vec takes 0 or 1 (got %lld)", value);
  g_vec.store(value, std::memory_order_relaxed);
  return FEDAGG_OK;
}

int fedagg_promote_wsum(const void* const* d_layers, const int* kinds, int nlists, const double* coeffs,
                        const uint64_t* numel, int L, double* d_flat, void* stream) {
  if (nlists < 1 || nlists > FEDAGG_FLAT_MAX_LISTS)
    return fail(FEDAGG_EINVAL, "promote wsum: nlists outside 1..FEDAGG_FLAT_MAX_LISTS (nlists=%lld)", nlists);
  if (!kinds) return fail(FEDAGG_EINVAL, "promote wsum: kinds is NULL");
  int kind16 = -1;
  uint32_t f64 = 0;
  for (int j = 0; j < nlists; ++j) {
    const int k = kinds[j];
    if (k == FEDAGG_F64) {
      f64 |= 1u << j;
    } else if (k == FEDAGG_F32) {
      return fail(FEDAGG_EINVAL, "promote wsum: list %lld is fp32 (fedagg_flat_wsum serves fp32 next to fp64)", j);
    } else if (!is_16bit_kind(k)) {
      return fail(FEDAGG_EINVAL, "promote wsum: list %lld has an unsupported kind", j);
    } else if (kind16 >= 0 && k != kind16) {
      return fail(FEDAGG_EINVAL, "promote wsum: F16 next to BF16 (list %lld)", j);
    } else {
      kind16 = k;
    }
  }
  if (kind16 < 0) return fail(FEDAGG_EINVAL, "promote wsum: no 16-bit list (fedagg_flat_wsum serves fp64 lists)");
  if (!f64) return fail(FEDAGG_EINVAL, "promote wsum: no fp64 list (fedagg_flat_wsum serves lists of one 16-bit kind)");
  return promote_launch(kind16 == FEDAGG_F16 ? promote_wsum_kernel<FEDAGG_F16> : promote_wsum_kernel<FEDAGG_BF16>,
                        d_layers, f64, nlists, coeffs, numel, L, d_flat, stream);
}

int fedagg_promote_increment(void* const* d_layers, int layer_kind, const uint64_t* numel, int L,
                             const double* d_flat, double multiplier, void* stream) {
  if (!is_16bit_kind(layer_kind))
    return fail(FEDAGG_EINVAL, "promote increment: layer_kind %lld is not FEDAGG_F16 / FEDAGG_BF16", layer_kind);
  return promote_launch(
      layer_kind == FEDAGG_F16 ? promote_increment_kernel<FEDAGG_F16> : promote_increment_kernel<FEDAGG_BF16>,
      static_cast<const void* const*>(static_cast<const void*>(d_layers)), 0u, 1, &multiplier, numel, L,
      d_flat, stream);
}

}  // extern "C"
