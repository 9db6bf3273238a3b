// topk.hip -- libfedagg_topk.so (include/fedagg_topk.h): the top-k sparse wire of FedAvg.  The
// client selects the k largest magnitudes of fl32(x + res) exactly, compacts them in index order
// and keeps the rest in res; the aggregator averages K such rows into a dense fp32 row.
//
// Selection.  A radix select on m = bits(r) & 0x7FFFFFFF in three histogram passes of 11, 10 and 10
// bits.  256 threads, a lane takes four consecutive elements at a time (a "quad": one 16-B load).
//   pass 1   fused: r = fl32(x + res) (never contracted), r stored over res, bin m >> 20 counted in
//            the workgroup's 2048 LDS bins (ds_add); the non-empty bins are flushed by integer adds
//   pick     one workgroup: lane t sums its share of the bins from the top, the shares are
//            prefixed through LDS, and the lane whose share holds rank k writes the bin (the radix
//            prefix) and the rank that remains inside it to d_state
//   pass 2/3 read res only; an element whose upper bits equal the prefix counts in 1024 bins
//   count    per tile of TK_TILE elements, the number of m >= max(t, 1): wave ballots, popcounts
//   scan     one workgroup: the tile counts become tile offsets in place, nnz goes to d_state
// Everything between the passes lives in device memory; the host reads d_state once, for nnz.
//
// Compaction.  A workgroup re-derives the flags of its tile (4 steps of 1024 elements, a lane's
// quad q = step * 256 + lane, so element order is step, wave, lane, element).  A lane's position is
//   tile offset + kept in earlier steps + kept in earlier waves of the step      (one LDS exchange)
//   + kept in lower lanes of the wave (popcount of each of the 4 ballots below the lane)
//   + kept among its own earlier elements
// so the row is ascending with no sort.  The quad goes back to res with +0.0 at the kept and the
// non-finite positions, only where something changed.
//
// FedAvg.  bounds: one thread per (sub-tile edge, client): lower_bound of the edge in the client's
// indices, laid out edge-major so a wave reads its 2 K bounds contiguously.  reduce: each WAVE owns
// a sub-tile of TK_SUB output elements in LDS (16 KiB; 4 waves per workgroup), zeroed to +0.0.
// It walks the clients in list order; its lanes take the client's entries inside the sub-tile, 64
// at a time, and do tile[i - base] = fl32(tile[i - base] + fl32(v * w_k)) as plain LDS
// read-modify-writes: a client's indices are unique, so lanes never meet inside one step, and the
// wave's LDS operations retire in program order, so client order is the reference's add order
// with no workgroup barrier and no atomics.  The bounds and the first 64 entries of the next
// TK_U clients are loaded ahead of the current group's adds (two register buffers).  The sub-tile
// leaves as 16-B non-temporal stores.  numel == 1 elements: a second small kernel, one workgroup
// per listed index, lane k binary-searches client k's row and lane 0 sums the K products with
// pw_leaf (NumPy's tree; K <= 128 is one leaf), absent terms as fl32(+0 * w_k).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "fedagg_topk.h"
#include "lib_error.h"
#include "pairwise_sum.h"

#define TK_THREADS 256                          // threads per workgroup
#define TK_WAVES (TK_THREADS / 64)
#define TK_STEPS 4                              // quads per lane and tile
#define TK_TILE (TK_THREADS * 4 * TK_STEPS)     // elements per select / compact tile (select_tile)
#define TK_SUB 4096                             // output elements per wave of the reduce kernel (sub_tile)
#define TK_U 4                                  // clients per load group (k_group)
#define TK_BINS1 2048                           // pass 1: the top 11 of the 31 magnitude bits
#define TK_BINS 1024                            // passes 2 and 3: 10 bits each
#define TK_HIST_WORDS (TK_BINS1 + 2 * TK_BINS)
#define TK_PW_IDX 64                            // numel == 1 indices per launch
#define TK_HIST_GRID 1024u                      // workgroups of a histogram pass (each flushes its bins once)
#define TK_GRID_CAP (1u << 18)

namespace {

using fedagg_internal::pw_leaf;
using fedagg_lib_error::fail;
constexpr auto check_launch = fedagg_lib_error::check_launch<FEDAGG_OK, FEDAGG_EHIP>;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t MAG = 0x7FFFFFFFu, INF = 0x7F800000u;
// d_state beyond the three public words
constexpr int ST_T = FEDAGG_TOPK_STATE_T, ST_NNZ = FEDAGG_TOPK_STATE_NNZ, ST_ERR = FEDAGG_TOPK_STATE_ERROR;
constexpr int ST_THR = 3, ST_PREFIX = 4, ST_RANK = 5;

// ------------------------------------------------------------------------------------
// The client side
// ------------------------------------------------------------------------------------

// The histograms, the state and nothing else: a kernel, so the call may be captured into a graph.
__global__ void __launch_bounds__(TK_THREADS) topk_clear_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ state) {
  for (int b = threadIdx.x; b < TK_HIST_WORDS; b += TK_THREADS) hist[b] = 0;
  if (threadIdx.x < FEDAGG_TOPK_STATE_WORDS) state[threadIdx.x] = 0;
}

// The four fp32 values of quad q of x (all inside the row, x 16-B aligned for its element size).
template <int KIND>
__device__ __forceinline__ void load_x4(const void* x, const uint64_t q, float (&v)[4]) {
  if constexpr (KIND == FEDAGG_F32) {
    const u32x4 r = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(x) + q);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __uint_as_float(r[j]);
  } else {  // bf16: the upper half of the fp32 pattern, exactly
    const u32x2 r = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(x) + q);
    v[0] = __uint_as_float(r[0] << 16);
    v[1] = __uint_as_float(r[0] & 0xFFFF0000u);
    v[2] = __uint_as_float(r[1] << 16);
    v[3] = __uint_as_float(r[1] & 0xFFFF0000u);
  }
}

template <int KIND>
__device__ __forceinline__ float load_x1(const void* x, const uint64_t i) {
  if constexpr (KIND == FEDAGG_F32) return reinterpret_cast<const float*>(x)[i];
  else return __uint_as_float((uint32_t) reinterpret_cast<const uint16_t*>(x)[i] << 16);
}

// Pass 1: r = fl32(x + res) over res in place, the top 11 magnitude bits counted.
template <int KIND>
__global__ void __launch_bounds__(TK_THREADS)
    topk_pass1_kernel(const void* __restrict__ x, float* __restrict__ res, const uint64_t M, uint32_t* __restrict__ hist,
                      const int vec) {
#pragma clang fp contract(off)
  __shared__ uint32_t bins[TK_BINS1];
  for (int b = threadIdx.x; b < TK_BINS1; b += TK_THREADS) bins[b] = 0;
  __syncthreads();
  const uint64_t nq = (M + 3) / 4;
  for (uint64_t q = (uint64_t)blockIdx.x * TK_THREADS + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * TK_THREADS) {
    const uint64_t e = q * 4;
    if (vec && e + 4 <= M) {
      float xv[4];
      load_x4<KIND>(x, q, xv);
      u32x4 r = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(res) + q);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float s = xv[j] + __uint_as_float(r[j]);
        r[j] = __float_as_uint(s);
        atomicAdd(&bins[(r[j] & MAG) >> 20], 1u);
      }
      reinterpret_cast<u32x4*>(res)[q] = r;
    } else {
      for (uint64_t i = e; i < M && i < e + 4; ++i) {
        const float s = load_x1<KIND>(x, i) + res[i];
        res[i] = s;
        atomicAdd(&bins[(__float_as_uint(s) & MAG) >> 20], 1u);
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < TK_BINS1; b += TK_THREADS)
    if (bins[b]) atomicAdd(&hist[b], bins[b]);
}

// f(bits, j) for the elements of quad q of res that lie inside the row.
template <typename F>
__device__ __forceinline__ void for_quad(const float* res, const uint64_t q, const uint64_t M, const int vec, const F& f) {
  const uint64_t e = q * 4;
  if (vec && e + 4 <= M) {
    const u32x4 r = reinterpret_cast<const u32x4*>(res)[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) f(r[j], j);
  } else {
    for (int j = 0; j < 4 && e + j < M; ++j) f(__float_as_uint(res[e + j]), j);
  }
}

// Passes 2 (SHIFT 10) and 3 (SHIFT 0): the elements whose bits above SHIFT + 10 equal the prefix,
// counted by their next 10 bits.
template <int SHIFT>
__global__ void __launch_bounds__(TK_THREADS)
    topk_pass_kernel(const float* __restrict__ res, const uint64_t M, const uint32_t* __restrict__ state,
                     uint32_t* __restrict__ hist, const int vec) {
  __shared__ uint32_t bins[TK_BINS];
  for (int b = threadIdx.x; b < TK_BINS; b += TK_THREADS) bins[b] = 0;
  __syncthreads();
  const uint32_t prefix = state[ST_PREFIX];
  const uint64_t nq = (M + 3) / 4;
  for (uint64_t q = (uint64_t)blockIdx.x * TK_THREADS + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * TK_THREADS) {
    for_quad(res, q, M, vec, [&](const uint32_t bits, int) {
      const uint32_t m = bits & MAG;
      if ((m >> (SHIFT + 10)) == prefix) atomicAdd(&bins[(m >> SHIFT) & (TK_BINS - 1)], 1u);
    });
  }
  __syncthreads();
  for (int b = threadIdx.x; b < TK_BINS; b += TK_THREADS)
    if (bins[b]) atomicAdd(&hist[b], bins[b]);
}

// One workgroup: the bin that holds the rank-th largest element, counted from the top bin down.
// PASS 1 takes the rank k and starts the prefix; 2 extends it; 3 completes t.
template <int NB, int PASS>
__global__ void __launch_bounds__(TK_THREADS)
    topk_pick_kernel(const uint32_t* __restrict__ hist, uint32_t* __restrict__ state, const uint32_t k) {
  __shared__ uint32_t part[TK_THREADS];
  constexpr int PER = NB / TK_THREADS;
  const int t = threadIdx.x;
  const uint32_t rank = PASS == 1 ? k : state[ST_RANK];
  const uint32_t prefix = PASS == 1 ? 0u : state[ST_PREFIX];
  uint32_t h[PER], s = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {  // lane t owns the bins NB - 1 - (t PER + j): lane 0 the topmost
    h[j] = hist[NB - 1 - (t * PER + j)];
    s += h[j];
  }
  part[t] = s;
  __syncthreads();
  uint32_t above = 0;  // elements in higher bins: at most M < 2^32 in all
  for (int i = 0; i < t; ++i) above += part[i];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (above < rank && rank - above <= h[j]) {  // exactly one lane and bin: rank <= the elements counted
      const uint32_t p = (prefix << (PASS == 1 ? 0 : 10)) | (uint32_t)(NB - 1 - (t * PER + j));
      state[ST_PREFIX] = p;
      state[ST_RANK] = rank - above;
      if (PASS == 3) {
        state[ST_T] = p;
        state[ST_THR] = p > 1u ? p : 1u;  // zeros are never sent
      }
    }
    above += h[j];
  }
}

// The kept elements of every tile.
__global__ void __launch_bounds__(TK_THREADS)
    topk_count_kernel(const float* __restrict__ res, const uint64_t M, const uint32_t* __restrict__ state,
                      uint32_t* __restrict__ tile_cnt, const int vec) {
  __shared__ uint32_t wsum[TK_WAVES];
  const uint32_t thr = state[ST_THR];
  const uint64_t ntiles = (M + TK_TILE - 1) / TK_TILE;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    uint32_t c = 0;  // wave-uniform
#pragma unroll
    for (int it = 0; it < TK_STEPS; ++it) {
      bool f[4] = {false, false, false, false};
      for_quad(res, tile * (TK_TILE / 4) + it * TK_THREADS + threadIdx.x, M, vec,
               [&](const uint32_t bits, const int j) { f[j] = (bits & MAG) >= thr; });
#pragma unroll
      for (int j = 0; j < 4; ++j) c += (uint32_t)__popcll(__ballot(f[j]));
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x / 64] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t s = 0;
      for (int w = 0; w < TK_WAVES; ++w) s += wsum[w];
      tile_cnt[tile] = s;
    }
    __syncthreads();  // wsum is rewritten by the next tile
  }
}

// One workgroup: the tile counts become exclusive tile offsets in place; nnz to the state.
__global__ void __launch_bounds__(TK_THREADS)
    topk_scan_kernel(uint32_t* __restrict__ tile_off, const uint64_t ntiles, uint32_t* __restrict__ state) {
  __shared__ uint32_t part[TK_THREADS];
  const uint64_t per = (ntiles + TK_THREADS - 1) / TK_THREADS;
  const uint64_t lo = threadIdx.x * per < ntiles ? threadIdx.x * per : ntiles;
  const uint64_t hi = lo + per < ntiles ? lo + per : ntiles;
  uint32_t s = 0;
  for (uint64_t i = lo; i < hi; ++i) s += tile_off[i];
  part[threadIdx.x] = s;
  __syncthreads();
  uint32_t above = 0;
  for (int i = 0; i < (int)threadIdx.x; ++i) above += part[i];
  for (uint64_t i = lo; i < hi; ++i) {
    const uint32_t c = tile_off[i];
    tile_off[i] = above;
    above += c;
  }
  if (threadIdx.x == TK_THREADS - 1) state[ST_NNZ] = above;  // the last lane's share ends the row
}

// The compaction, and the new residual.
__global__ void __launch_bounds__(TK_THREADS)
    topk_compact_kernel(float* __restrict__ res, const uint64_t M, const uint32_t* __restrict__ tile_off,
                        uint32_t* __restrict__ state, const uint32_t nnz, uint32_t* __restrict__ idx,
                        float* __restrict__ val, const int vec) {
  __shared__ uint32_t wt[TK_STEPS][TK_WAVES];
  if (state[ST_NNZ] != nnz) {  // the caller's nnz sized idx and val: nothing is written
    if (blockIdx.x == 0 && threadIdx.x == 0) state[ST_ERR] = 1;
    return;
  }
  const uint32_t thr = state[ST_THR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
  const uint64_t below = (1ull << lane) - 1;
  const uint64_t ntiles = (M + TK_TILE - 1) / TK_TILE;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    uint32_t r[TK_STEPS][4];
    uint32_t before[TK_STEPS];  // kept in the lower lanes of this wave, per step
#pragma unroll
    for (int it = 0; it < TK_STEPS; ++it) {
#pragma unroll
      for (int j = 0; j < 4; ++j) r[it][j] = 0;  // past the row: magnitude 0, never kept
      for_quad(res, tile * (TK_TILE / 4) + it * TK_THREADS + threadIdx.x, M, vec,
               [&](const uint32_t bits, const int j) { r[it][j] = bits; });
      uint32_t b = 0, total = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint64_t bal = __ballot((r[it][j] & MAG) >= thr);
        b += (uint32_t)__popcll(bal & below);
        total += (uint32_t)__popcll(bal);
      }
      before[it] = b;
      if (lane == 0) wt[it][wave] = total;
    }
    __syncthreads();
    uint32_t p0 = tile_off[tile];
#pragma unroll
    for (int it = 0; it < TK_STEPS; ++it) {
      uint32_t p = p0 + before[it];
#pragma unroll
      for (int w = 0; w < TK_WAVES; ++w) {
        if (w < wave) p += wt[it][w];
        p0 += wt[it][w];
      }
      const uint64_t q = tile * (TK_TILE / 4) + it * TK_THREADS + threadIdx.x;
      const uint64_t e = q * 4;
      u32x4 z;
      bool changed = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t m = r[it][j] & MAG;
        const bool kept = m >= thr;
        if (kept) {
          if (p < nnz) {  // always, for the res the selection counted
            idx[p] = (uint32_t)(e + j);
            val[p] = __uint_as_float(r[it][j]);
          }
          ++p;
        }
        const bool drop = kept || m >= INF;
        z[j] = drop ? 0u : r[it][j];
        changed |= drop;
      }
      if (changed) {
        if (vec && e + 4 <= M) {
          reinterpret_cast<u32x4*>(res)[q] = z;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (e + j < M && z[j] != r[it][j]) res[e + j] = 0.0f;
        }
      }
    }
    __syncthreads();  // wt is rewritten by the next tile
  }
}

// ------------------------------------------------------------------------------------
// The aggregator
// ------------------------------------------------------------------------------------

struct TkArgs {
  const uint32_t* idx[FEDAGG_TOPK_KMAX];
  const float* val[FEDAGG_TOPK_KMAX];
  uint32_t nnz[FEDAGG_TOPK_KMAX];
  float w[FEDAGG_TOPK_KMAX];
};

// The first position of row `idx` (n ascending entries) whose index is >= target.
__device__ __forceinline__ uint32_t lower_bound(const uint32_t* idx, const uint32_t n, const uint64_t target) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((uint64_t)idx[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// bnd[e K + k]: where sub-tile edge e (element e TK_SUB) falls in client k's row; e in [0, nsub].
__global__ void __launch_bounds__(TK_THREADS)
    topk_bounds_kernel(const TkArgs a, const int K, const uint64_t nsub, uint32_t* __restrict__ bnd) {
  const uint64_t g = (uint64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (g >= (nsub + 1) * (uint64_t)K) return;
  const uint64_t e = g / (uint64_t)K;
  const int k = (int)(g % (uint64_t)K);
  bnd[g] = lower_bound(a.idx[k], a.nnz[k], e * TK_SUB);
}

// Orders the wave's LDS accesses across its lanes for the compiler; the hardware keeps them in
// program order.  No instruction of its own.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// tile[i - base] = fl32(tile[i - base] + fl32(v * w)); an index outside the sub-tile (a row that is
// not ascending) is dropped, never written.
__device__ __forceinline__ void add_entry(float* tile, const uint64_t base, const uint32_t i, const float v, const float w) {
#pragma clang fp contract(off)
  const uint64_t d = (uint64_t)i - base;
  if (d < TK_SUB) {
    const float p = v * w;
    tile[d] = tile[d] + p;
  }
}

// What a lane holds of TK_U clients for one sub-tile: their bounds and its entry of the first 64.
struct Group {
  uint32_t lo[TK_U], hi[TK_U], i[TK_U];
  float v[TK_U];
};

__device__ __forceinline__ void load_group(const TkArgs& a, const uint32_t* bnd, const int K, const uint64_t s,
                                           const int k0, const int lane, Group& g) {
#pragma unroll
  for (int u = 0; u < TK_U; ++u) {
    g.lo[u] = bnd[s * K + k0 + u];
    g.hi[u] = bnd[(s + 1) * K + k0 + u];
  }
#pragma unroll
  for (int u = 0; u < TK_U; ++u) {
    const uint32_t j = g.lo[u] + lane;
    g.i[u] = 0;
    g.v[u] = 0.0f;
    if (j < g.hi[u]) {
      g.i[u] = __builtin_nontemporal_load(a.idx[k0 + u] + j);
      g.v[u] = __builtin_nontemporal_load(a.val[k0 + u] + j);
    }
  }
}

// Client k's entries [lo, hi) onto the sub-tile; (i0, v0) is the lane's entry of the first 64.
__device__ __forceinline__ void add_client(const TkArgs& a, float* tile, const uint64_t base, const int k,
                                           const uint32_t lo, const uint32_t hi, const uint32_t i0, const float v0,
                                           const int lane) {
  const float w = a.w[k];
  uint32_t j = lo + lane;
  if (j < hi) add_entry(tile, base, i0, v0, w);
  for (j += 64; j < hi; j += 64) add_entry(tile, base, a.idx[k][j], a.val[k][j], w);  // a row denser than 64 per sub-tile
  wave_lds_order();  // the next client may meet this one's indices in other lanes
}

__device__ __forceinline__ void add_group(const TkArgs& a, float* tile, const uint64_t base, const int k0, const int lane,
                                          const Group& g) {
#pragma unroll
  for (int u = 0; u < TK_U; ++u) add_client(a, tile, base, k0 + u, g.lo[u], g.hi[u], g.i[u], g.v[u], lane);
}

__global__ void __launch_bounds__(TK_THREADS)
    topk_fedavg_kernel(const TkArgs a, const int K, const uint64_t M, const uint32_t* __restrict__ bnd,
                       float* __restrict__ out, const int out16) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float tiles[TK_WAVES][TK_SUB];
  const int lane = threadIdx.x & 63;
  float* tile = tiles[threadIdx.x / 64];
  const uint64_t nsub = (M + TK_SUB - 1) / TK_SUB;
  for (uint64_t s = (uint64_t)blockIdx.x * TK_WAVES + threadIdx.x / 64; s < nsub; s += (uint64_t)gridDim.x * TK_WAVES) {
    const uint64_t base = s * TK_SUB;
    for (int q = lane; q < TK_SUB / 4; q += 64) {  // NumPy seeds add.reduce with +0.0
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[4 * q + j] = 0.0f;
    }
    wave_lds_order();

    int k = 0;
    if (K >= TK_U) {
      Group ga, gb;
      load_group(a, bnd, K, s, 0, lane, ga);
      for (;;) {
        const bool mb = k + 2 * TK_U <= K;
        if (mb) load_group(a, bnd, K, s, k + TK_U, lane, gb);
        add_group(a, tile, base, k, lane, ga);
        k += TK_U;
        if (!mb) break;
        const bool ma = k + 2 * TK_U <= K;
        if (ma) load_group(a, bnd, K, s, k + TK_U, lane, ga);
        add_group(a, tile, base, k, lane, gb);
        k += TK_U;
        if (!ma) break;
      }
    }
    for (; k < K; ++k) {
      const uint32_t lo = bnd[s * K + k], hi = bnd[(s + 1) * K + k];
      const uint32_t j = lo + lane;
      uint32_t i0 = 0;
      float v0 = 0.0f;
      if (j < hi) {
        i0 = a.idx[k][j];
        v0 = a.val[k][j];
      }
      add_client(a, tile, base, k, lo, hi, i0, v0, lane);
    }

    for (int q = lane; q < TK_SUB / 4; q += 64) {
      const uint64_t e = base + 4 * (uint64_t)q;
      if (e >= M) break;
      u32x4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = __float_as_uint(tile[4 * q + j]);
      if (out16 && e + 4 <= M) {
        __builtin_nontemporal_store(r, reinterpret_cast<u32x4*>(out + e));
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (e + j < M) out[e + j] = __uint_as_float(r[j]);
      }
    }
    wave_lds_order();  // the reads above, before the next sub-tile's zeros
  }
}

struct PwIdx {
  uint32_t i[TK_PW_IDX];
};

// One workgroup per listed index, lane k the term of client k.
__global__ void __launch_bounds__(FEDAGG_TOPK_KMAX)
    topk_pairwise_kernel(const TkArgs a, const PwIdx pi, const int K, float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ float term[FEDAGG_TOPK_KMAX];
  const uint32_t i = pi.i[blockIdx.x];
  const int k = threadIdx.x;
  if (k < K) {
    const uint32_t n = a.nnz[k];
    const uint32_t j = lower_bound(a.idx[k], n, i);
    const float x = (j < n && a.idx[k][j] == i) ? a.val[k][j] : 0.0f;  // an absent element is +0.0
    term[k] = x * a.w[k];
  }
  __syncthreads();
  if (k == 0) {
    auto get = [&](int64_t c) -> float { return term[c]; };
    out[i] = 0.0f + pw_leaf<float>(get, 0, K);  // NumPy's reduction adds the tree's root to +0.0
  }
}

unsigned grid_for(uint64_t items, unsigned cap) {
  uint64_t g = items < 1 ? 1 : items;
  return (unsigned)(g > cap ? cap : g);
}

uint64_t div_up(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

size_t select_ws_bytes(uint64_t M) { return (size_t)((TK_HIST_WORDS + div_up(M, TK_TILE) + 1) * 4 + 255) / 256 * 256; }
size_t fedavg_ws_bytes(uint64_t M, int K) { return (size_t)(((div_up(M, TK_SUB) + 1) * (uint64_t)K * 4 + 255) / 256 * 256); }

template <int KIND>
int launch_select(const void* d_x, float* d_res, uint64_t M, uint32_t k, uint32_t* ws, uint32_t* d_state, hipStream_t st) {
  uint32_t* h1 = ws;
  uint32_t* h2 = ws + TK_BINS1;
  uint32_t* h3 = h2 + TK_BINS;
  uint32_t* tile_cnt = ws + TK_HIST_WORDS;
  const uint64_t ntiles = div_up(M, TK_TILE);
  const int xa = KIND == FEDAGG_F32 ? 15 : 7;  // a quad of x is 16 or 8 bytes
  const int rvec = (reinterpret_cast<uintptr_t>(d_res) & 15u) == 0;
  const int vec = rvec && (reinterpret_cast<uintptr_t>(d_x) & xa) == 0;
  const dim3 hist_grid(grid_for(div_up(div_up(M, 4), TK_THREADS), TK_HIST_GRID)), one(1), th(TK_THREADS);
  int rc;
  hipLaunchKernelGGL(topk_clear_kernel, one, th, 0, st, ws, d_state);
  if ((rc = check_launch("topk clear kernel"))) return rc;
  hipLaunchKernelGGL(topk_pass1_kernel<KIND>, hist_grid, th, 0, st, d_x, d_res, M, h1, vec);
  if ((rc = check_launch("topk pass 1 kernel"))) return rc;
  hipLaunchKernelGGL((topk_pick_kernel<TK_BINS1, 1>), one, th, 0, st, h1, d_state, k);
  if ((rc = check_launch("topk pick 1 kernel"))) return rc;
  hipLaunchKernelGGL(topk_pass_kernel<10>, hist_grid, th, 0, st, d_res, M, d_state, h2, rvec);
  if ((rc = check_launch("topk pass 2 kernel"))) return rc;
  hipLaunchKernelGGL((topk_pick_kernel<TK_BINS, 2>), one, th, 0, st, h2, d_state, k);
  if ((rc = check_launch("topk pick 2 kernel"))) return rc;
  hipLaunchKernelGGL(topk_pass_kernel<0>, hist_grid, th, 0, st, d_res, M, d_state, h3, rvec);
  if ((rc = check_launch("topk pass 3 kernel"))) return rc;
  hipLaunchKernelGGL((topk_pick_kernel<TK_BINS, 3>), one, th, 0, st, h3, d_state, k);
  if ((rc = check_launch("topk pick 3 kernel"))) return rc;
  hipLaunchKernelGGL(topk_count_kernel, dim3(grid_for(ntiles, TK_GRID_CAP)), th, 0, st, d_res, M, d_state, tile_cnt, rvec);
  if ((rc = check_launch("topk count kernel"))) return rc;
  hipLaunchKernelGGL(topk_scan_kernel, one, th, 0, st, tile_cnt, ntiles, d_state);
  return check_launch("topk scan kernel");
}

bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" {

int fedagg_topk_abi_version(void) { return FEDAGG_TOPK_ABI_VERSION; }
const char* fedagg_topk_last_error(void) { return fedagg_lib_error::g_error; }

int fedagg_topk_blocking(int* select_tile, int* sub_tile, int* k_group, int* threads) {
  if (select_tile) *select_tile = TK_TILE;
  if (sub_tile) *sub_tile = TK_SUB;
  if (k_group) *k_group = TK_U;
  if (threads) *threads = TK_THREADS;
  return FEDAGG_OK;
}

int fedagg_topk_workspace(uint64_t M, int K, size_t* select_bytes, size_t* fedavg_bytes) {
  if (M >= (1ull << 32)) return fail(FEDAGG_EINVAL, "topk workspace: M must be below 2^32 (M=%llu)", (unsigned long long)M);
  if (K < 0 || K > FEDAGG_TOPK_KMAX)
    return fail(FEDAGG_EINVAL, "topk workspace: K is outside [0, FEDAGG_TOPK_KMAX] (K=%lld)", (long long)K);
  if (select_bytes) *select_bytes = select_ws_bytes(M);
  if (fedavg_bytes) *fedavg_bytes = fedavg_ws_bytes(M, K);
  return FEDAGG_OK;
}

int fedagg_topk_select(int in_kind, const void* d_x, float* d_res, uint64_t M, uint64_t k, void* d_ws, size_t ws_bytes,
                       uint32_t* d_state, void* stream) {
  if (in_kind != FEDAGG_F32 && in_kind != FEDAGG_BF16)
    return fail(FEDAGG_EINVAL, "topk select: in_kind %lld is not FEDAGG_F32 / FEDAGG_BF16", (long long)in_kind);
  if (M == 0) return FEDAGG_OK;
  if (M >= (1ull << 32)) return fail(FEDAGG_EINVAL, "topk select: M must be below 2^32 (M=%llu)", (unsigned long long)M);
  if (k < 1 || k > M)
    return fail(FEDAGG_EINVAL, "topk select: k is outside [1, M] (k=%llu, M=%llu)", (unsigned long long)k,
                (unsigned long long)M);
  if (!d_x) return fail(FEDAGG_EINVAL, "topk select: d_x is NULL");
  if (!d_res) return fail(FEDAGG_EINVAL, "topk select: d_res is NULL");
  if (!d_ws) return fail(FEDAGG_EINVAL, "topk select: d_ws is NULL");
  if (!d_state) return fail(FEDAGG_EINVAL, "topk select: d_state is NULL");
  const uint64_t esz = in_kind == FEDAGG_F32 ? 4 : 2;
  if (reinterpret_cast<uintptr_t>(d_x) & (esz - 1)) return fail(FEDAGG_EINVAL, "topk select: d_x is not aligned to its element");
  if (reinterpret_cast<uintptr_t>(d_res) & 3u) return fail(FEDAGG_EINVAL, "topk select: d_res is not 4-B aligned");
  if (reinterpret_cast<uintptr_t>(d_ws) & 15u) return fail(FEDAGG_EINVAL, "topk select: d_ws is not 16-B aligned");
  if (reinterpret_cast<uintptr_t>(d_state) & 15u) return fail(FEDAGG_EINVAL, "topk select: d_state is not 16-B aligned");
  if (overlap(d_res, 4 * M, d_x, esz * M)) return fail(FEDAGG_EINVAL, "topk select: d_res overlaps d_x");
  if (ws_bytes < select_ws_bytes(M))
    return fail(FEDAGG_EINVAL, "topk select: ws_bytes is %llu, the selection needs %llu", (unsigned long long)ws_bytes,
                (unsigned long long)select_ws_bytes(M));
  if (in_kind == FEDAGG_F32)
    return launch_select<FEDAGG_F32>(d_x, d_res, M, (uint32_t)k, static_cast<uint32_t*>(d_ws), d_state, (hipStream_t)stream);
  return launch_select<FEDAGG_BF16>(d_x, d_res, M, (uint32_t)k, static_cast<uint32_t*>(d_ws), d_state, (hipStream_t)stream);
}

int fedagg_topk_compact(float* d_res, uint64_t M, const void* d_ws, uint32_t* d_state, uint64_t nnz, uint32_t* d_idx,
                        float* d_val, void* stream) {
  if (M == 0) return FEDAGG_OK;
  if (M >= (1ull << 32)) return fail(FEDAGG_EINVAL, "topk compact: M must be below 2^32 (M=%llu)", (unsigned long long)M);
  if (nnz > M)
    return fail(FEDAGG_EINVAL, "topk compact: nnz is above M (nnz=%llu, M=%llu)", (unsigned long long)nnz,
                (unsigned long long)M);
  if (!d_res) return fail(FEDAGG_EINVAL, "topk compact: d_res is NULL");
  if (!d_ws) return fail(FEDAGG_EINVAL, "topk compact: d_ws is NULL");
  if (!d_state) return fail(FEDAGG_EINVAL, "topk compact: d_state is NULL");
  if (nnz && !d_idx) return fail(FEDAGG_EINVAL, "topk compact: d_idx is NULL with nnz > 0");
  if (nnz && !d_val) return fail(FEDAGG_EINVAL, "topk compact: d_val is NULL with nnz > 0");
  if (reinterpret_cast<uintptr_t>(d_res) & 3u) return fail(FEDAGG_EINVAL, "topk compact: d_res is not 4-B aligned");
  if (reinterpret_cast<uintptr_t>(d_idx) & 3u) return fail(FEDAGG_EINVAL, "topk compact: d_idx is not 4-B aligned");
  if (reinterpret_cast<uintptr_t>(d_val) & 3u) return fail(FEDAGG_EINVAL, "topk compact: d_val is not 4-B aligned");
  const int vec = (reinterpret_cast<uintptr_t>(d_res) & 15u) == 0;
  const uint32_t* tile_off = static_cast<const uint32_t*>(d_ws) + TK_HIST_WORDS;
  hipLaunchKernelGGL(topk_compact_kernel, dim3(grid_for(div_up(M, TK_TILE), TK_GRID_CAP)), dim3(TK_THREADS), 0,
                     (hipStream_t)stream, d_res, M, tile_off, d_state, (uint32_t)nnz, d_idx, d_val, vec);
  return check_launch("topk compact kernel");
}

int fedagg_topk_fedavg(const uint32_t* const* d_idx, const float* const* d_val, const uint64_t* nnz, const float* h_w,
                       int K, uint64_t M, const uint64_t* h_pw_idx, int P, void* d_ws, size_t ws_bytes, float* d_out,
                       void* stream) {
  if (K <= 0) return fail(FEDAGG_EINVAL, "topk fedavg: K must be positive (K=%lld)", (long long)K);
  if (K > FEDAGG_TOPK_KMAX)
    return fail(FEDAGG_EINVAL, "topk fedavg: at most FEDAGG_TOPK_KMAX clients per call (K=%lld)", (long long)K);
  if (!d_idx) return fail(FEDAGG_EINVAL, "topk fedavg: d_idx is NULL");
  if (!d_val) return fail(FEDAGG_EINVAL, "topk fedavg: d_val is NULL");
  if (!nnz) return fail(FEDAGG_EINVAL, "topk fedavg: nnz is NULL");
  if (!h_w) return fail(FEDAGG_EINVAL, "topk fedavg: h_w is NULL");
  if (P < 0) return fail(FEDAGG_EINVAL, "topk fedavg: P is negative (P=%lld)", (long long)P);
  if (P > 0 && !h_pw_idx) return fail(FEDAGG_EINVAL, "topk fedavg: h_pw_idx is NULL with P > 0");
  if (M == 0) return FEDAGG_OK;
  if (M >= (1ull << 32)) return fail(FEDAGG_EINVAL, "topk fedavg: M must be below 2^32 (M=%llu)", (unsigned long long)M);
  TkArgs a;
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < K; ++k) {
    if (nnz[k] > M)
      return fail(FEDAGG_EINVAL, "topk fedavg: row %lld holds more than M entries (nnz=%llu)", (long long)k,
                  (unsigned long long)nnz[k]);
    if (nnz[k] && !d_idx[k]) return fail(FEDAGG_EINVAL, "topk fedavg: index row %lld is NULL", (long long)k);
    if (nnz[k] && !d_val[k]) return fail(FEDAGG_EINVAL, "topk fedavg: value row %lld is NULL", (long long)k);
    if (reinterpret_cast<uintptr_t>(d_idx[k]) & 3u)
      return fail(FEDAGG_EINVAL, "topk fedavg: index row %lld is not 4-B aligned", (long long)k);
    if (reinterpret_cast<uintptr_t>(d_val[k]) & 3u)
      return fail(FEDAGG_EINVAL, "topk fedavg: value row %lld is not 4-B aligned", (long long)k);
    a.idx[k] = d_idx[k];
    a.val[k] = d_val[k];
    a.nnz[k] = (uint32_t)nnz[k];
    a.w[k] = h_w[k];
  }
  if (!d_ws) return fail(FEDAGG_EINVAL, "topk fedavg: d_ws is NULL");
  if (reinterpret_cast<uintptr_t>(d_ws) & 3u) return fail(FEDAGG_EINVAL, "topk fedavg: d_ws is not 4-B aligned");
  if (ws_bytes < fedavg_ws_bytes(M, K))
    return fail(FEDAGG_EINVAL, "topk fedavg: ws_bytes is %llu, the bounds need %llu", (unsigned long long)ws_bytes,
                (unsigned long long)fedavg_ws_bytes(M, K));
  if (!d_out) return fail(FEDAGG_EINVAL, "topk fedavg: d_out is NULL");
  if (reinterpret_cast<uintptr_t>(d_out) & 3u) return fail(FEDAGG_EINVAL, "topk fedavg: d_out is not 4-B aligned");
  for (int p = 0; p < P; ++p)
    if (h_pw_idx[p] >= M) return fail(FEDAGG_EINVAL, "topk fedavg: numel == 1 index %lld is out of range", (long long)p);

  hipStream_t st = (hipStream_t)stream;
  uint32_t* bnd = static_cast<uint32_t*>(d_ws);
  const uint64_t nsub = div_up(M, TK_SUB);
  hipLaunchKernelGGL(topk_bounds_kernel, dim3((unsigned)div_up((nsub + 1) * (uint64_t)K, TK_THREADS)), dim3(TK_THREADS), 0,
                     st, a, K, nsub, bnd);
  int rc = check_launch("topk bounds kernel");
  if (rc) return rc;
  const int out16 = (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0;
  hipLaunchKernelGGL(topk_fedavg_kernel, dim3(grid_for(div_up(nsub, TK_WAVES), TK_GRID_CAP)), dim3(TK_THREADS), 0, st, a,
                     K, M, bnd, d_out, out16);
  if ((rc = check_launch("topk fedavg kernel"))) return rc;
  for (int p0 = 0; p0 < P; p0 += TK_PW_IDX) {
    PwIdx pi;
    memset(&pi, 0, sizeof(pi));
    const int n = P - p0 < TK_PW_IDX ? P - p0 : TK_PW_IDX;
    for (int p = 0; p < n; ++p) pi.i[p] = (uint32_t)h_pw_idx[p0 + p];
    hipLaunchKernelGGL(topk_pairwise_kernel, dim3(n), dim3(FEDAGG_TOPK_KMAX), 0, st, a, pi, K, d_out);
    if ((rc = check_launch("topk pairwise kernel"))) return rc;
  }
  return FEDAGG_OK;
}

}  // extern "C"
