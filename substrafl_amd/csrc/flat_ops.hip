// flat_ops.hip -- client-side flat-bucket ops: the producer /
// consumer of the buckets, i.e. weight_manager's per-layer torch loops (weight_manager.py:103-238)
// done as one launch over up to SEG_GROUP layers.  Workgroup b serves layer l with
// block_start[l] <= b < block_start[l+1], elements [(b - block_start[l]) * SEG_CHUNK, ...).
// Semantics follow the reference's torch ops bit for bit.  torch computes every op in fp32
// (opmath) for fp32, fp16 and bf16 tensors and rounds the op's result once to the tensor's type
// T (fl_T; the identity for fp32); a Python scalar is rounded to fp32:
//   weighted_sum_parameters (:182-212): Python sum() from int 0 over param * coeff, i.e.
//     p_j = fl_T(x_j * fl32(c_j)); acc = fl_T(0.0f + p_0) (-0 becomes +0); acc = fl_T(acc + p_j)
//   increment_parameters (:103-137):  w = fl_T(w + fl_T(fl32(mult) * u))
//   get_parameters / set_parameters: plain copies.
// Operand sets with an fp64 member follow torch's promotion in flat_seg_kernel.
// Bit parity needs every product and sum rounded separately: the file is compiled with
// -ffp-contract=off AND every kernel body and per-element helper carries
// `#pragma clang fp contract(off)`.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <type_traits>

#include "fedagg_internal.h"

using fedagg_internal::check_launch;
using fedagg_internal::fail;

namespace {

#define SEG_GROUP 32
#define SEG_CHUNK 8192  // elements per workgroup

struct SegArgs {
  const void* p[FEDAGG_FLAT_MAX_LISTS][SEG_GROUP];  // list-major layer pointers
  uint64_t n[SEG_GROUP];
  uint64_t flat_off[SEG_GROUP];
  uint32_t block_start[SEG_GROUP + 1];
  double coeff[FEDAGG_FLAT_MAX_LISTS];
  uint32_t f64;  // flat_seg_kernel: bit j says list j is fp64
  int vec;       // flat_typed_kernel: the "flat_vec" knob
  int nl, nlists;
};

__device__ __forceinline__ int seg_of_block(const SegArgs& a, uint32_t b) {
  int l = 0;
  while (l + 1 < a.nl && a.block_start[l + 1] <= b) ++l;  // scalar, <= SEG_GROUP steps
  return l;
}

template <typename T>
__device__ __forceinline__ T* layer(const SegArgs& a, int j, int l) {
  return const_cast<T*>(static_cast<const T*>(a.p[j][l]));
}

// ------------------------------------------------------------------------------------
// Operand sets with an fp64 member (Scaffold's client side: the server control variate arrives
// as fp64).  The launcher sends a call here only when a list or the bucket is fp64, and then the
// bucket always is: a copy has one kind, the result of a weighted sum has the promoted kind, and
// the increment's parameters are fp32, so its update is what is fp64.
// ------------------------------------------------------------------------------------

// torch's ``tensor * python_float``: fp32 tensors compute in fp32 with the scalar rounded to
// fp32, fp64 tensors in fp64.  Returned in double (exact for the fp32 product).
__device__ __forceinline__ double seg_product(const void* p, uint64_t i, bool is64, double c) {
#pragma clang fp contract(off)
  if (is64) return static_cast<const double*>(p)[i] * c;
  return (double)(static_cast<const float*>(p)[i] * (float)c);
}

// op 0: gather (flat = p0, fp64), 2: wsum (flat = sum() of p_j * c_j, lists fp32 or fp64 per
// SegArgs::f64), 3: increment (p0 = p0 + c0 * flat, p0 fp32).  The op runs in fp64 once either
// side is fp64, as torch's promotion has it.
template <int OP>
__global__ void __launch_bounds__(FA_BLOCK) flat_seg_kernel(const SegArgs a, void* __restrict__ flat) {
#pragma clang fp contract(off)
  static_assert(OP == 0 || OP == 2 || OP == 3, "the ABI has no fp64 scatter");
  const int l = seg_of_block(a, blockIdx.x);
  const uint64_t base = (uint64_t)(blockIdx.x - a.block_start[l]) * SEG_CHUNK;
  const uint64_t n = a.n[l];
  double* f = static_cast<double*>(flat) + a.flat_off[l];
  for (uint64_t i = base + threadIdx.x; i < base + SEG_CHUNK && i < n; i += FA_BLOCK) {
    if constexpr (OP == 0) {
      f[i] = layer<double>(a, 0, l)[i];
    } else if constexpr (OP == 2) {
      // Python sum() from int 0: 0 + p_0 (-0 becomes +0), then acc + p_j in the promoted type
      bool acc64 = a.f64 & 1u;
      double acc = seg_product(a.p[0][l], i, acc64, a.coeff[0]);
      acc = acc64 ? 0.0 + acc : (double)(0.0f + (float)acc);
      for (int j = 1; j < a.nlists; ++j) {
        const bool is64 = (a.f64 >> j) & 1u;
        const double t = seg_product(a.p[j][l], i, is64, a.coeff[j]);
        acc64 = acc64 || is64;
        acc = acc64 ? acc + t : (double)((float)acc + (float)t);
      }
      f[i] = acc;
    } else {
      // w += m * u with w fp32 and u fp64: fl32(w + fl64(m * u))
      float* w = layer<float>(a, 0, l);
      const double t = a.coeff[0] * f[i];
      w[i] = (float)((double)w[i] + t);
    }
  }
}

// ------------------------------------------------------------------------------------
// fp32, fp16 and bf16: one kernel over the element kind K.  16-bit elements are handled as their
// bit patterns; widen<K> is exact, round_to<K> is torch's rounding of an fp32 result to K.
// ------------------------------------------------------------------------------------
template <int K>
using elem_t = std::conditional_t<K == FEDAGG_F32, float, uint16_t>;

template <int K>
__device__ __forceinline__ float widen(elem_t<K> b) {
  if constexpr (K == FEDAGG_F32) return b;
  else if constexpr (K == FEDAGG_F16) return (float)__builtin_bit_cast(_Float16, b);
  else return __uint_as_float((uint32_t)b << 16);
}

// fp32 -> K: round to nearest even, overflow to +-inf, NaN stays NaN (quiet bit set)
template <int K>
__device__ __forceinline__ elem_t<K> round_to(float f) {
  if constexpr (K == FEDAGG_F32) {
    return f;
  } else if constexpr (K == FEDAGG_F16) {
    // The fp32 value and the converted bits each pass through a register of their own, so the
    // rounding is one plain v_cvt_f16_f32 of the fp32 result: the compiler neither folds the
    // multiply before it into a mixed-precision fma nor pairs two conversions into a packed one.
    asm("" : "+v"(f));
    uint32_t r = __builtin_bit_cast(uint16_t, (_Float16)f);
    asm("" : "+v"(r));
    return (uint16_t)r;
  } else {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  }
}

// a + b where a NaN in a wins: of two NaN operands the hardware returns the payload of the first
// source, and the compiler commutes a plain ``a + b`` as it likes, differently in the wide loop
// and in the tail.  Spelled out, a result does not depend on which of the two loops made it,
// NaN payloads included.  (Plain C++ on purpose: inline asm is convergent in device code, and a
// loop that holds one is no longer unrolled.)
__device__ __forceinline__ float add_in_order(float a, float b) {
#pragma clang fp contract(off)
  const float r = a + b;
  return a != a ? __uint_as_float(__float_as_uint(a) | 0x00400000u) : r;  // a, quieted
}

// Each op's arithmetic, once: the wide loop and the tail of flat_typed_kernel both call these.
// c and m are the Python scalars as torch takes them, rounded to fp32.
template <int K>
__device__ __forceinline__ elem_t<K> wsum_first(elem_t<K> x, float c) {
#pragma clang fp contract(off)
  const elem_t<K> p = round_to<K>(widen<K>(x) * c);
  return round_to<K>(add_in_order(0.0f, widen<K>(p)));  // Python sum() starts from int 0: -0 becomes +0
}
template <int K>
__device__ __forceinline__ elem_t<K> wsum_next(elem_t<K> acc, elem_t<K> x, float c) {
#pragma clang fp contract(off)
  const elem_t<K> p = round_to<K>(widen<K>(x) * c);
  return round_to<K>(add_in_order(widen<K>(acc), widen<K>(p)));
}
// w + m * u.  The update u has kind K, except FLAT32: the increment of a bf16 model by the
// engine's fp32 average.  torch's type promotion defines that in-place add as the fp32 sum
// rounded once, t = fl32(m * u) staying fp32, and that is what its CPU kernels and its generic
// device kernel give.  torch on ROCm (2.10) serves an aligned contiguous ``bf16 += fp32`` with a
// type-specialised vectorised kernel (ATen/native/cuda/CUDALoops.cuh, rt_binary_specializations
// {BFloat16, BFloat16, float}) whose loads convert both inputs to the OUTPUT type: in every full
// block of FLAT_TORCH_MIXED_BLOCK elements of the tensor the fp32 operand is rounded to bf16
// before the add; the remainder of the tensor goes through the generic kernel.  The reference's
// tensors are whole aligned allocations (one ``.to(device)`` per layer), so a layer's leading
// full blocks get two roundings there, and ``twice`` reproduces that here.
#define FLAT_TORCH_MIXED_BLOCK 16384  // vectorized_templated_config: 512 threads x 32 elements
static_assert(FLAT_TORCH_MIXED_BLOCK % SEG_CHUNK == 0, "a chunk lies inside one torch block or outside all of them");
template <int K, bool FLAT32>
__device__ __forceinline__ elem_t<K> increment(elem_t<K> w, std::conditional_t<FLAT32, float, elem_t<K>> u, float m,
                                               bool twice) {
#pragma clang fp contract(off)
  float t;
  if constexpr (FLAT32) t = m * u;
  else t = m * widen<K>(u);
  if (!FLAT32 || twice) t = widen<K>(round_to<K>(t));
  return round_to<K>(add_in_order(widen<K>(w), t));
}

// W elements of T moved as one access declared A-byte aligned.
template <typename T, int W, int A>
struct Vec {
  typedef T type __attribute__((ext_vector_type(W), aligned(A)));
};

// op 0: gather (flat = p0), 1: scatter (p0 = flat, fp32 only), 2: wsum, 3: increment, over layers
// of kind K.  The bucket has kind K too, except FLAT32: a bf16 model incremented by an fp32 bucket.
// A chunk moves 16 B (W elements) per lane and access, its last < W elements one element per
// lane, consecutive lanes on consecutive elements.  A layer's slice of the bucket starts
// wherever the previous layers end, so 16-B accesses of the slice are declared 4-B aligned:
// gfx950 serves unaligned dwordx4 loads and stores, a wave still touches one contiguous KiB
// (plus at most one extra line).
//   fp32:   layers are declared 4-B aligned as well; every layer goes wide.
//   16-bit: a layer goes wide when its pointers are all 16-B aligned AND its slice of a 16-bit
//           bucket starts at an even element (4-B aligned).  An fp32 bucket (FLAT32) is always
//           4-B aligned and read with two 16-B loads.  Every other layer -- a slice at an odd
//           element offset never sees a multi-dword access -- goes element by element like the
//           tail.  There is no wide form for a 2-B aligned address: eight 2-byte accesses of one
//           lane would be merged into one wide access by the compiler.
// Without SegArgs::vec every layer goes element by element.
template <int OP, int K, bool FLAT32>
__global__ void __launch_bounds__(FA_BLOCK) flat_typed_kernel(const SegArgs a, void* __restrict__ flat) {
#pragma clang fp contract(off)
  static_assert(!FLAT32 || (OP == 3 && K == FEDAGG_BF16), "an fp32 bucket next to 16-bit layers: bf16 increment only");
  static_assert(OP != 1 || K == FEDAGG_F32, "the ABI has no 16-bit scatter");
  using T = elem_t<K>;
  using U = std::conditional_t<FLAT32, float, T>;  // the bucket's element
  constexpr int W = 16 / sizeof(T);
  using LayerVec = typename Vec<T, W, (K == FEDAGG_F32 ? 4 : 16)>::type;
  using SliceVec = typename Vec<U, W, 4>::type;
  const int l = seg_of_block(a, blockIdx.x);
  const uint64_t base = (uint64_t)(blockIdx.x - a.block_start[l]) * SEG_CHUNK;
  const uint64_t n = a.n[l];
  const uint64_t end = base + SEG_CHUNK < n ? base + SEG_CHUNK : n;
  U* f = static_cast<U*>(flat) + a.flat_off[l];
  T* p0 = layer<T>(a, 0, l);
  float cf[FEDAGG_FLAT_MAX_LISTS];
#pragma unroll
  for (int j = 0; j < FEDAGG_FLAT_MAX_LISTS; ++j) cf[j] = (float)a.coeff[j];  // torch rounds the scalar
  bool wide = a.vec;
  if constexpr (K != FEDAGG_F32) {
    uintptr_t bits = 0;
    for (int j = 0; j < a.nlists; ++j) bits |= reinterpret_cast<uintptr_t>(a.p[j][l]);
    wide = wide && (bits & 15u) == 0 && (FLAT32 || (reinterpret_cast<uintptr_t>(f) & 3u) == 0);
  }
  // FLAT32 only: chunks inside the layer's leading full torch blocks (a block is two chunks)
  const bool twice = FLAT32 && base < (n & ~(uint64_t)(FLAT_TORCH_MIXED_BLOCK - 1));
  uint64_t tail = base + threadIdx.x;  // where the element-by-element loop starts
  if (wide) {
    const uint64_t vend = base + ((end - base) & ~(uint64_t)(W - 1));
    for (uint64_t i = base + W * (uint64_t)threadIdx.x; i < vend; i += W * (uint64_t)FA_BLOCK) {
      LayerVec* v0 = reinterpret_cast<LayerVec*>(p0 + i);
      SliceVec* vf = reinterpret_cast<SliceVec*>(f + i);
      if constexpr (OP == 0) {
        *vf = *v0;
      } else if constexpr (OP == 1) {
        *v0 = *vf;
      } else if constexpr (OP == 2) {
        LayerVec x = *v0;
        SliceVec acc;
#pragma unroll
        for (int e = 0; e < W; ++e) acc[e] = wsum_first<K>(x[e], cf[0]);
        for (int j = 1; j < a.nlists; ++j) {
          x = *reinterpret_cast<const LayerVec*>(layer<T>(a, j, l) + i);
#pragma unroll
          for (int e = 0; e < W; ++e) acc[e] = wsum_next<K>(acc[e], x[e], cf[j]);
        }
        *vf = acc;
      } else {
        LayerVec w = *v0;
        const SliceVec u = *vf;
#pragma unroll
        for (int e = 0; e < W; ++e) w[e] = increment<K, FLAT32>(w[e], u[e], cf[0], twice);
        *v0 = w;
      }
    }
    tail = vend + threadIdx.x;
  }
  for (uint64_t i = tail; i < end; i += FA_BLOCK) {
    if constexpr (OP == 0) {
      f[i] = p0[i];
    } else if constexpr (OP == 1) {
      p0[i] = f[i];
    } else if constexpr (OP == 2) {
      T acc = wsum_first<K>(p0[i], cf[0]);
      for (int j = 1; j < a.nlists; ++j) acc = wsum_next<K>(acc, layer<T>(a, j, l)[i], cf[j]);
      f[i] = acc;
    } else {
      p0[i] = increment<K, FLAT32>(p0[i], f[i], cf[0], twice);
    }
  }
}

// ------------------------------------------------------------------------------------
// Launch.  A per-op front (plan_*) checks the operand kinds and names the kernel; flat_launch
// checks the rest, packs SegArgs group by group and launches.
// ------------------------------------------------------------------------------------
struct FlatPlan {
  void (*kernel)(const SegArgs, void*);  // nullptr: the kinds were refused and the error text is set
  uint32_t f64;                          // SegArgs::f64
  unsigned layer_align, flat_align;      // bytes every layer pointer / the bucket must be aligned to
};
const FlatPlan kRefused = {nullptr, 0, 1, 1};

bool is_16bit_kind(int k) { return k == FEDAGG_F16 || k == FEDAGG_BF16; }

template <int OP, int K, bool FLAT32 = false>
FlatPlan typed_plan() {
  constexpr unsigned al = K == FEDAGG_F32 ? 1 : 2;  // fp32 pointers are taken as they come
  return {flat_typed_kernel<OP, K, FLAT32>, 0, al, FLAT32 ? 4 : al};
}
template <int OP>
FlatPlan f64_plan(uint32_t f64) {
  return {flat_seg_kernel<OP>, f64, 1, 1};
}
FlatPlan refuse(const char* fmt, long long b = 0) {
  fail(FEDAGG_EINVAL, fmt, b);
  return kRefused;
}

// gather (OP 0) / scatter (OP 1): layers and bucket of one kind
template <int OP>
FlatPlan plan_copy(int kind) {
  if (kind == FEDAGG_F32) return typed_plan<OP, FEDAGG_F32>();
  if constexpr (OP == 0) {
    if (kind == FEDAGG_F64) return f64_plan<0>(1u);
    if (is_16bit_kind(kind)) return typed_plan<0, FEDAGG_F16>();  // a copy of bit patterns: one instance serves both kinds
  }
  return refuse("flat copy: unsupported kind %lld", kind);
}

// kinds == NULL: every list fp32
FlatPlan plan_wsum(const int* kinds, int nlists, int flat_kind) {
  if (nlists < 1 || nlists > FEDAGG_FLAT_MAX_LISTS) return refuse("flat op: invalid argument (nlists=%lld)", nlists);
  bool any16 = is_16bit_kind(flat_kind);
  uint32_t f64 = 0;
  for (int j = 0; j < nlists; ++j) {
    const int k = kinds ? kinds[j] : FEDAGG_F32;
    any16 = any16 || is_16bit_kind(k);
    if (k == FEDAGG_F64) f64 |= 1u << j;
  }
  if (any16) {  // every list and the result of ONE 16-bit kind; torch's promotion is not done here
    for (int j = 0; j < nlists; ++j)
      if ((kinds ? kinds[j] : FEDAGG_F32) != flat_kind)
        return refuse("flat wsum: 16-bit lists take lists and a result of one kind (list %lld)", j);
    return flat_kind == FEDAGG_F16 ? typed_plan<2, FEDAGG_F16>() : typed_plan<2, FEDAGG_BF16>();
  }
  if (flat_kind != FEDAGG_F32 && flat_kind != FEDAGG_F64)
    return refuse("flat op: the flat bucket must be fp32 or fp64 (kind %lld)", flat_kind);
  for (int j = 0; j < nlists; ++j)
    if (kinds && kinds[j] != FEDAGG_F32 && kinds[j] != FEDAGG_F64) return refuse("flat op: list %lld is not fp32/fp64", j);
  if ((f64 != 0) != (flat_kind == FEDAGG_F64))
    return refuse("flat wsum: the result kind must be the promoted kind of the lists");
  return f64 ? f64_plan<2>(f64) : typed_plan<2, FEDAGG_F32>();
}

FlatPlan plan_increment(int layer_kind, int flat_kind) {
  if (layer_kind == FEDAGG_F64) return refuse("flat increment: parameters must be fp32");
  if (layer_kind == FEDAGG_F32) {
    if (flat_kind == FEDAGG_F32) return typed_plan<3, FEDAGG_F32>();
    if (flat_kind == FEDAGG_F64) return f64_plan<3>(0);
    return refuse("flat op: the flat bucket must be fp32 or fp64 (kind %lld)", flat_kind);
  }
  if (layer_kind == FEDAGG_F16 && flat_kind == FEDAGG_F16) return typed_plan<3, FEDAGG_F16>();
  if (layer_kind == FEDAGG_BF16 && flat_kind == FEDAGG_BF16) return typed_plan<3, FEDAGG_BF16>();
  if (layer_kind == FEDAGG_BF16 && flat_kind == FEDAGG_F32) return typed_plan<3, FEDAGG_BF16, true>();
  return refuse("flat increment: unsupported (layer, flat) kinds (flat kind %lld)", flat_kind);
}

// ptrs is list-major [nlists][L]; coeffs == NULL: all 1.
int flat_launch(const FlatPlan& plan, const void* const* ptrs, int nlists, const double* coeffs,
                const uint64_t* numel, int L, const void* flat, void* stream) {
  if (!plan.kernel) return FEDAGG_EINVAL;
  if (L < 0 || (L > 0 && (!ptrs || !numel || !flat))) return fail(FEDAGG_EINVAL, "flat op: invalid argument (L=%lld)", L);
  if (reinterpret_cast<uintptr_t>(flat) & (plan.flat_align - 1)) return fail(FEDAGG_EINVAL, "flat op: misaligned flat bucket");
  uint64_t off = 0;
  for (int l0 = 0; l0 < L; l0 += SEG_GROUP) {
    const int nl = (L - l0) < SEG_GROUP ? (L - l0) : SEG_GROUP;
    SegArgs a;
    memset(&a, 0, sizeof(a));
    a.nl = nl;
    a.nlists = nlists;
    a.f64 = plan.f64;
    a.vec = fedagg_internal::flat_vec();
    for (int j = 0; j < nlists; ++j) a.coeff[j] = coeffs ? coeffs[j] : 1.0;
    uint64_t blocks = 0;
    for (int l = 0; l < nl; ++l) {
      for (int j = 0; j < nlists; ++j) {
        a.p[j][l] = ptrs[(size_t)j * L + l0 + l];
        if (!a.p[j][l] && numel[l0 + l]) return fail(FEDAGG_EINVAL, "flat op: NULL layer pointer %lld", l0 + l);
        if (reinterpret_cast<uintptr_t>(a.p[j][l]) & (plan.layer_align - 1))
          return fail(FEDAGG_EINVAL, "flat op: misaligned layer pointer %lld", l0 + l);
      }
      a.n[l] = numel[l0 + l];
      a.flat_off[l] = off;
      a.block_start[l] = (uint32_t)blocks;
      off += numel[l0 + l];
      blocks += (numel[l0 + l] + SEG_CHUNK - 1) / SEG_CHUNK;
    }
    a.block_start[nl] = (uint32_t)blocks;
    if (blocks == 0) continue;
    hipLaunchKernelGGL(plan.kernel, dim3((unsigned)blocks), dim3(FA_BLOCK), 0, (hipStream_t)stream, a,
                       const_cast<void*>(flat));
    const int rc = check_launch("flat op kernel");
    if (rc) return rc;
  }
  return FEDAGG_OK;
}

const void* const* as_lists(const void* p) { return static_cast<const void* const*>(p); }

}  // namespace

extern "C" {

int fedagg_flat_gather(const void* const* d_layers, int kind, const uint64_t* numel, int L, void* d_flat,
                       void* stream) {
  return flat_launch(plan_copy<0>(kind), d_layers, 1, nullptr, numel, L, d_flat, stream);
}
int fedagg_flat_wsum(const void* const* d_layers, const int* kinds, int nlists, const double* coeffs,
                     const uint64_t* numel, int L, void* d_flat, int flat_kind, void* stream) {
  return flat_launch(plan_wsum(kinds, nlists, flat_kind), d_layers, nlists, coeffs, numel, L, d_flat, stream);
}
int fedagg_flat_increment_kind(void* const* d_layers, int layer_kind, const uint64_t* numel, int L,
                               const void* d_flat, int flat_kind, double multiplier, void* stream) {
  if (!is_16bit_kind(layer_kind))  // fedagg_flat_increment keeps fp32 parameters
    return fail(FEDAGG_EINVAL, "flat increment: unsupported (layer, flat) kinds (flat kind %lld)", flat_kind);
  return flat_launch(plan_increment(layer_kind, flat_kind), as_lists(d_layers), 1, &multiplier, numel, L, d_flat,
                     stream);
}
int fedagg_flat_increment(float* const* d_layers, const uint64_t* numel, int L, const void* d_flat, int flat_kind,
                          double multiplier, void* stream) {
  return flat_launch(plan_increment(FEDAGG_F32, flat_kind), as_lists(d_layers), 1, &multiplier, numel, L, d_flat,
                     stream);
}

int fedagg_flat_gather_f32(const float* const* d_layers, const uint64_t* numel, int L, float* d_flat,
                           void* stream) {
  return fedagg_flat_gather(as_lists(d_layers), FEDAGG_F32, numel, L, d_flat, stream);
}
int fedagg_flat_scatter_f32(float* const* d_layers, const uint64_t* numel, int L, const float* d_flat, void* stream) {
  return flat_launch(plan_copy<1>(FEDAGG_F32), as_lists(d_layers), 1, nullptr, numel, L, d_flat, stream);
}
int fedagg_flat_wsum_f32(const float* const* d_layers, int nlists, const double* coeffs, const uint64_t* numel, int L,
                         float* d_flat, void* stream) {
  return fedagg_flat_wsum(as_lists(d_layers), nullptr, nlists, coeffs, numel, L, d_flat, FEDAGG_F32, stream);
}
int fedagg_flat_increment_f32(float* const* d_layers, const uint64_t* numel, int L, const float* d_flat,
                              double multiplier, void* stream) {
  return fedagg_flat_increment(d_layers, numel, L, d_flat, FEDAGG_F32, multiplier, stream);
}

}  // extern "C"
