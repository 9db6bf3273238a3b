// krum.hip -- libfedagg_krum.so (include/fedagg_krum.h): G = X X^T in fp64 over K client rows, the
// device half of Krum and multi-Krum.
//
// Every other kernel of the engine streams K rows into one output row.  This one streams them into a
// K x K matrix: a GEMM with K <= 128 and M in the hundreds of millions, on v_mfma_f64_16x16x4_f64.
//
// One operand, two roles.  The instruction's A operand of a block of 16 clients puts client l & 15
// and k-slot l >> 4 in lane l, and its B operand of a block of 16 clients has the same map.  So one
// register image of a block is A for the block's tile row and B for its tile column, a diagonal tile
// passes the same register twice, and a block is loaded once per step however many tiles it feeds.
// The C/D map is register q of lane l = C[(l >> 4) + 4 q][l & 15] (csrc/dense_internal.h).
//
// k in any order.  A sum over k does not care which element sits in which k-slot as long as A and B
// agree, and here they are the same registers.  A lane therefore takes one 16-B load of VEC
// consecutive elements of its client's row (4 fp32, 8 bf16), widens them in registers and each of
// the VEC values becomes its k-slot's value in one of VEC operand images.  Nothing is transposed.
//
// The step.  A workgroup of 4 waves covers KR_CHUNK = 64 elements of all 16 NB rows per step
// (NB = ceil(K / 16) blocks).  The loads of a step are (block, 16-element group) pairs dealt to the
// waves round robin; the widened values go to the LDS panel[block][slot][lane], KR_SLOTS = 16 operand
// images of 64 doubles per block, written and read with consecutive lanes on consecutive doubles.
// Every wave then reads the images of the blocks its tiles need and issues one MFMA per tile and
// image.  The next step's loads are issued before this step's MFMAs and wait in registers.  Every row
// is read from HBM once per call, with non-temporal loads.
//
// Who owns what.  The upper triangle has T = NB (NB + 1) / 2 tiles, up to 36: too many accumulators
// for one wave, too few at small K to keep four waves busy.  The unit of work is (tile, k-part): the
// 16 images of a step are dealt to KS k-parts (KS = 4 up to 32 clients, 2 up to 64, 1 beyond), and
// unit u = tile * KS + kpart belongs to wave u % 4.  With KS = 4 every wave holds every tile for a
// quarter of the images; with KS = 1 the tiles are dealt round robin, 9 to a wave at K = 128.  Unit
// to wave to register is a compile-time map per NB, so 8 clients do not pay for 128.
//
// Split-M without atomics.  Workgroup g takes steps [g share, (g + 1) share) and writes its U = T KS
// partial tiles to d_ws.  gram_finish adds, for each entry of the upper triangle, the partials in
// the order g = 0 .., kpart = 0 .. (in 16 runs, then the runs in order: one thread's chain of every
// partial is latency, not bandwidth) and writes the entry and its mirror image (a diagonal tile's
// r <= c half only, so both triangles carry the very same double).  share, the grid and the runs are
// functions of (K, M) alone.
//
// Tails and padding never touch memory: a lane's group at or past M is +0.0 without a load, a group
// that straddles M loads its elements below M one by one, and a lane of a client >= K holds a null
// row and loads nothing.  Rows that are not all 16-B aligned load every group element by element
// into the same registers: the same element in the same slot of the same workgroup, so the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <utility>

#include "fedagg_krum.h"
#include "lib_error.h"

#define KR_THREADS 256
#define KR_WAVES 4
#define KR_CHUNK 64                // elements of every row per workgroup step
#define KR_SLOTS (KR_CHUNK / 4)    // operand images per block and step: one MFMA per tile and image
#define KR_VEC_F32 4
#define KR_VEC_BF16 8
#define KR_MIN_STEPS 8             // a workgroup's share is at least this many steps (but for the last)
#define KR_TILE_BYTES (256 * 8)    // one partial tile in d_ws
#define KR_FIN_SLICES 16           // runs an entry's partials are added in (gram_finish)

namespace {

using fedagg_lib_error::fail;
constexpr auto check_launch = fedagg_lib_error::check_launch<FEDAGG_OK, FEDAGG_EHIP>;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

struct KrArgs {
  const void* row[FEDAGG_KRUM_MAX_K];
};

constexpr int tiles_of(int nb) { return nb * (nb + 1) / 2; }
constexpr int ksplit_of(int nb) { return nb <= 2 ? 4 : (nb <= 4 ? 2 : 1); }
constexpr int units_of(int nb) { return tiles_of(nb) * ksplit_of(nb); }
// workgroups at most: enough to fill the device several times at the LDS a panel of nb blocks takes
constexpr int grid_max_of(int nb) { return nb <= 4 ? 1024 : 512; }

// Tile t of the upper triangle, rows first: (0,0) (0,1) .. (0,nb-1) (1,1) ..
__host__ __device__ constexpr int tile_row(int nb, int t) {
  int bi = 0;
  while (t >= nb - bi) { t -= nb - bi; ++bi; }
  return bi;
}
__host__ __device__ constexpr int tile_col(int nb, int t) {
  int bi = 0;
  while (t >= nb - bi) { t -= nb - bi; ++bi; }
  return bi + t;
}

// How M is split: nsteps steps of KR_CHUNK, `share` steps per workgroup, `grid` workgroups.
struct Split {
  uint64_t nsteps, share, grid;
};
inline Split split_of(int nb, uint64_t M) {
  Split s;
  s.nsteps = (M + KR_CHUNK - 1) / KR_CHUNK;
  if (s.nsteps == 0) return s.share = 0, s.grid = 0, s;
  uint64_t g0 = (s.nsteps + KR_MIN_STEPS - 1) / KR_MIN_STEPS;
  if (g0 > (uint64_t)grid_max_of(nb)) g0 = grid_max_of(nb);
  s.share = (s.nsteps + g0 - 1) / g0;
  s.grid = (s.nsteps + s.share - 1) / s.share;
  return s;
}

// One lane's group of VEC elements of its row from element g on, as 16 bytes: zeros past M and for a
// null row (a client >= K), one 16-B load where the call's rows allow it, else element by element.
template <int KIND>
__device__ __forceinline__ u32x4 load_group(const uint8_t* row, const uint64_t g, const uint64_t M, const bool aligned) {
  constexpr int VEC = KIND == FEDAGG_BF16 ? KR_VEC_BF16 : KR_VEC_F32;
  u32x4 r = {0u, 0u, 0u, 0u};
  if (row == nullptr || g >= M) return r;
  if (aligned && g + VEC <= M) {
    if constexpr (KIND == FEDAGG_BF16) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row + g * 2));
    else return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row + g * 4));
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    if (g + e < M) {
      if constexpr (KIND == FEDAGG_BF16) {
        const uint32_t h = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(row) + g + e);
        r[e / 2] |= h << (16 * (e & 1));
      } else {
        r[e] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(row) + g + e);
      }
    }
  }
  return r;
}

// Element e of a loaded group, widened exactly.
template <int KIND>
__device__ __forceinline__ double widen(const u32x4 r, const int e) {
  if constexpr (KIND == FEDAGG_BF16) {
    const uint32_t w = r[e / 2];
    return (double)__uint_as_float((e & 1) ? (w & 0xFFFF0000u) : (w << 16));
  } else {
    return (double)__uint_as_float(r[e]);
  }
}

// Unit I of wave WAVE: u = WAVE + 4 I, its tile's row and column block; one MFMA on the step's image v.
template <int NB, int WAVE, int I>
__device__ __forceinline__ void unit_mfma(f64x4* acc, const double (&v)[NB]) {
  constexpr int T = (WAVE + KR_WAVES * I) / ksplit_of(NB);
  constexpr int BI = tile_row(NB, T), BJ = tile_col(NB, T);
  acc[I] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[BI], v[BJ], acc[I], 0, 0, 0);
}

template <int NB, int WAVE, int... I>
__device__ __forceinline__ void units_mfma(f64x4* acc, const double (&v)[NB], std::integer_sequence<int, I...>) {
  (unit_mfma<NB, WAVE, I>(acc, v), ...);
}

// The MFMAs of one step for wave WAVE: its k-part's images (every KS-th from WAVE % KS on), for each
// the blocks its tiles name (a block no tile of the wave names is not read: the load is dead code).
template <int NB, int WAVE>
__device__ __forceinline__ void wave_step(f64x4* acc, const double (*panel)[KR_SLOTS][64], const int lane) {
  constexpr int KS = ksplit_of(NB), U = units_of(NB);
  constexpr int MINE = (U - WAVE + KR_WAVES - 1) / KR_WAVES;  // units of this wave
  if constexpr (MINE > 0) {
#pragma unroll
    for (int s = WAVE % KS; s < KR_SLOTS; s += KS) {
      double v[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) v[b] = panel[b][s][lane];
      units_mfma<NB, WAVE>(acc, v, std::make_integer_sequence<int, MINE>{});
    }
  }
}

// Workgroup g: steps [g share, min((g + 1) share, nsteps)) of KR_CHUNK elements; its U partial tiles
// to ws[g][u][lane][q].
template <int KIND, int NB>
__global__ void __launch_bounds__(KR_THREADS)
    gram_kernel(const KrArgs a, const int K, const uint64_t M, const uint64_t nsteps, const uint64_t share, const int aligned,
                double* __restrict__ ws) {
  constexpr int VEC = KIND == FEDAGG_BF16 ? KR_VEC_BF16 : KR_VEC_F32;
  constexpr int J = KR_CHUNK / (4 * VEC);  // 16-element groups of a block per step: a (block, group) pair is one wave load
  constexpr int P = NB * J, PPW = (P + KR_WAVES - 1) / KR_WAVES;
  constexpr int U = units_of(NB), UPW = (U + KR_WAVES - 1) / KR_WAVES;
  static_assert(J * VEC == KR_SLOTS && KR_SLOTS % ksplit_of(NB) == 0, "a pair fills VEC images, the k-parts share them evenly");
  __shared__ double panel[NB][KR_SLOTS][64];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, q = lane >> 4;

  // pair i of this wave: p = wave + 4 i, block p / J, group p % J; the lane's row of it, null past K or P
  const uint8_t* row[PPW];
  uint32_t goff[PPW];  // the lane's first element within the step
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int p = wave + KR_WAVES * i;
    const int client = (p / J) * 16 + c;
    row[i] = (p < P && client < K) ? static_cast<const uint8_t*>(a.row[client & (FEDAGG_KRUM_MAX_K - 1)]) : nullptr;
    goff[i] = (uint32_t)(((p % J) * 4 + q) * VEC);
  }

  f64x4 acc[UPW];
#pragma unroll
  for (int i = 0; i < UPW; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};

  const uint64_t first = (uint64_t)blockIdx.x * share;
  const uint64_t last = first + share < nsteps ? first + share : nsteps;
  u32x4 raw[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) raw[i] = load_group<KIND>(row[i], first * KR_CHUNK + goff[i], M, aligned != 0);

  for (uint64_t st = first; st < last; ++st) {
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int p = wave + KR_WAVES * i;
      if (p < P) {  // wave-uniform
        double(*img)[64] = panel[p / J] + (p % J) * VEC;
#pragma unroll
        for (int e = 0; e < VEC; ++e) img[e][lane] = widen<KIND>(raw[i], e);
      }
    }
    __syncthreads();
    if (st + 1 < last) {  // the next step's loads, in flight behind this step's MFMAs
#pragma unroll
      for (int i = 0; i < PPW; ++i) raw[i] = load_group<KIND>(row[i], (st + 1) * KR_CHUNK + goff[i], M, aligned != 0);
    }
    switch (wave) {
      case 0: wave_step<NB, 0>(acc, panel, lane); break;
      case 1: wave_step<NB, 1>(acc, panel, lane); break;
      case 2: wave_step<NB, 2>(acc, panel, lane); break;
      default: wave_step<NB, 3>(acc, panel, lane); break;
    }
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < UPW; ++i) {
    const int u = wave + KR_WAVES * i;
    if (u < U) {
      double* dst = ws + (((uint64_t)blockIdx.x * U + u) * 64 + lane) * 4;
      dst[0] = acc[i][0]; dst[1] = acc[i][1]; dst[2] = acc[i][2]; dst[3] = acc[i][3];
    }
  }
}

// Workgroup b: 16 entries of tile b / 16 of the upper triangle.  An entry's partials, numbered
// n = workgroup * ks + k-part, are cut into KR_FIN_SLICES contiguous runs of equal length; thread
// (slice, entry) adds its run in ascending n, then one thread per entry adds the 16 runs in ascending
// order and writes the entry and its mirror image.  The tree is a function of the partial count alone.
__global__ void __launch_bounds__(KR_THREADS)
    gram_finish(const double* __restrict__ ws, const uint64_t grid, const int nb, const int ks, const int K,
                double* __restrict__ G) {
  __shared__ double run[KR_FIN_SLICES][16];
  const int t = blockIdx.x / 16;
  const int e = (blockIdx.x % 16) * 16 + (threadIdx.x & 15), s = threadIdx.x >> 4;  // e = lane * 4 + register
  const int l = e >> 2, q = e & 3;
  const int bi = tile_row(nb, t), bj = tile_col(nb, t);
  const int r = (l >> 4) + 4 * q, c = l & 15;
  const int i = bi * 16 + r, j = bj * 16 + c;
  const bool mine = i < K && j < K && (bi != bj || r <= c);
  const uint64_t units = (uint64_t)tiles_of(nb) * ks, parts = grid * ks;
  const uint64_t len = (parts + KR_FIN_SLICES - 1) / KR_FIN_SLICES;
  const uint64_t n0 = s * len < parts ? s * len : parts, n1 = n0 + len < parts ? n0 + len : parts;
  const double* src = ws + (uint64_t)t * ks * 256 + e;
  double sum = 0.0;
  if (mine) {
#pragma unroll 8
    for (uint64_t n = n0; n < n1; ++n) sum = sum + src[((n / ks) * units + n % ks) * 256];
  }
  run[s][threadIdx.x & 15] = sum;
  __syncthreads();
  if (mine && s == 0) {
    double total = 0.0;
#pragma unroll
    for (int k = 0; k < KR_FIN_SLICES; ++k) total = total + run[k][threadIdx.x];
    G[(uint64_t)i * K + j] = total;
    G[(uint64_t)j * K + i] = total;
  }
}

template <int KIND, int NB>
void launch(const KrArgs& a, int K, uint64_t M, const Split& s, int aligned, double* ws, hipStream_t stream) {
  hipLaunchKernelGGL((gram_kernel<KIND, NB>), dim3((unsigned)s.grid), dim3(KR_THREADS), 0, stream, a, K, M, s.nsteps,
                     s.share, aligned, ws);
}

template <int KIND>
void dispatch(int nb, const KrArgs& a, int K, uint64_t M, const Split& s, int aligned, double* ws, hipStream_t stream) {
  switch (nb) {
    case 1: return launch<KIND, 1>(a, K, M, s, aligned, ws, stream);
    case 2: return launch<KIND, 2>(a, K, M, s, aligned, ws, stream);
    case 3: return launch<KIND, 3>(a, K, M, s, aligned, ws, stream);
    case 4: return launch<KIND, 4>(a, K, M, s, aligned, ws, stream);
    case 5: return launch<KIND, 5>(a, K, M, s, aligned, ws, stream);
    case 6: return launch<KIND, 6>(a, K, M, s, aligned, ws, stream);
    case 7: return launch<KIND, 7>(a, K, M, s, aligned, ws, stream);
    default: return launch<KIND, 8>(a, K, M, s, aligned, ws, stream);
  }
}

int check_size(const char* what, int K, uint64_t M) {
  if (K <= 0 || K > FEDAGG_KRUM_MAX_K)
    return fail(FEDAGG_EINVAL, "%s: K is outside [1, FEDAGG_KRUM_MAX_K] (K=%lld)", what, (long long)K);
  if (M > (1ull << 44)) return fail(FEDAGG_EINVAL, "%s: M is above 2^44 (M=%llu)", what, (unsigned long long)M);
  return FEDAGG_OK;
}

uint64_t ws_bytes_of(int nb, uint64_t M) { return split_of(nb, M).grid * units_of(nb) * KR_TILE_BYTES; }

}  // namespace

extern "C" {

int fedagg_krum_abi_version(void) { return FEDAGG_KRUM_ABI_VERSION; }
const char* fedagg_krum_last_error(void) { return fedagg_lib_error::g_error; }

int fedagg_krum_blocking(int* chunk_elems, int* vec_f32, int* vec_bf16) {
  if (chunk_elems) *chunk_elems = KR_CHUNK;
  if (vec_f32) *vec_f32 = KR_VEC_F32;
  if (vec_bf16) *vec_bf16 = KR_VEC_BF16;
  return FEDAGG_OK;
}

int fedagg_krum_ws_bytes(int K, uint64_t M, uint64_t* bytes) {
  if (int rc = check_size("krum ws_bytes", K, M)) return rc;
  if (!bytes) return fail(FEDAGG_EINVAL, "krum ws_bytes: bytes is NULL");
  *bytes = ws_bytes_of((K + 15) / 16, M);
  return FEDAGG_OK;
}

int fedagg_krum_gram(const void* const* d_rows, int kind, int K, uint64_t M, void* d_ws, uint64_t ws_bytes, double* d_G,
                     void* stream) {
  if (int rc = check_size("krum gram", K, M)) return rc;
  if (kind != FEDAGG_F32 && kind != FEDAGG_BF16)
    return fail(FEDAGG_EINVAL, "krum gram: kind %lld is not FEDAGG_F32 / FEDAGG_BF16", (long long)kind);
  if (!d_rows) return fail(FEDAGG_EINVAL, "krum gram: d_rows is NULL");
  const uintptr_t esz = kind == FEDAGG_F32 ? 4 : 2;
  uintptr_t low = 0;
  KrArgs a;
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < K; ++k) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(d_rows[k]);
    if (!p) return fail(FEDAGG_EINVAL, "krum gram: row %lld is NULL", (long long)k);
    if (p & (esz - 1)) return fail(FEDAGG_EINVAL, "krum gram: row %lld is not aligned to its element", (long long)k);
    low |= p;
    a.row[k] = d_rows[k];
  }
  if (!d_G) return fail(FEDAGG_EINVAL, "krum gram: d_G is NULL");
  if (reinterpret_cast<uintptr_t>(d_G) & 7u) return fail(FEDAGG_EINVAL, "krum gram: d_G is not 8-B aligned");
  if (!d_ws) return fail(FEDAGG_EINVAL, "krum gram: d_ws is NULL");
  if (reinterpret_cast<uintptr_t>(d_ws) & 15u) return fail(FEDAGG_EINVAL, "krum gram: d_ws is not 16-B aligned");
  const int nb = (K + 15) / 16;
  const uint64_t need = ws_bytes_of(nb, M);
  if (ws_bytes < need)
    return fail(FEDAGG_EINVAL, "krum gram: ws_bytes = %llu is below fedagg_krum_ws_bytes = %llu",
                (unsigned long long)ws_bytes, (unsigned long long)need);

  const Split s = split_of(nb, M);
  double* ws = static_cast<double*>(d_ws);
  if (s.grid) {
    const int aligned = (low & 15u) == 0;
    if (kind == FEDAGG_F32) dispatch<FEDAGG_F32>(nb, a, K, M, s, aligned, ws, (hipStream_t)stream);
    else dispatch<FEDAGG_BF16>(nb, a, K, M, s, aligned, ws, (hipStream_t)stream);
    if (int rc = check_launch("krum gram kernel")) return rc;
  }
  hipLaunchKernelGGL(gram_finish, dim3((unsigned)tiles_of(nb) * 16), dim3(KR_THREADS), 0, (hipStream_t)stream, ws, s.grid, nb,
                     ksplit_of(nb), K, d_G);
  return check_launch("krum finish kernel");
}

}  // extern "C"
