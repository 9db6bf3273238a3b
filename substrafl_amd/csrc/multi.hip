// multi.hip -- one process, several GPUs: the parameter-range FedAvg of an aggregate task in ONE
// C call (SURVEY.md §8(b) "fa_multi_init / fa_reduce_sharded_*", §8(e) primary partitioning).
//
// A Substra aggregate task is one OS process (remote/register/register.py:96 runs one
// function.py), so a host that wants the node's GPUs drives them from one process.  The Python
// drop-in does that in substrafl_amd/multi_device.py (MultiDeviceEngine); this is the same plan for
// a host in another language, without Python:
//   * the flat bucket range [0, M) is cut into one contiguous, 512-element-aligned shard per
//     device (sharding.shard_bounds);
//   * one thread and one private session per shard (repeated device indices get their own
//     sessions, so a one-GPU box exercises the sharded path), its pack workers and pinned ring
//     placed on the GPU's NUMA node (multi_device.host_placement);
//   * the thread streams its shard through its GPU in sub-ranges sized to the free HBM
//     (out-of-core past 288 GB): stage bytes [lo, hi) of every client's row over the GPU's own
//     PCIe link (fedagg_session_stage_range), run the bucket kernel with the client order and the
//     numel == 1 patch of the elements it owns, fetch its slice straight into the caller's output.
// Every output element is computed by the single-GPU kernel's arithmetic, so the result is bit-
// identical to fedagg_fedavg_* over the whole range and to the reference (fed_avg.py:217-222): no
// collective, no re-association.  bf16 rows (fedagg_multi_fedavg_bf16) run the same plan with
// 2-byte elements in and fp32 out: K * 2 + 4 bytes of HBM per element of a sub-range.
//
// Scaffold runs on the same plan one bucket per call (fedagg_multi_scaffold_bucket): rows of any
// float kind staged as they are, fedagg_scaffold_bucket per sub-range, and the clients' copies of c
// compared on the pack workers while copy 0 of the sub-range is staged (scaffold.py:193-196,
// 262-263, 293).

#include <hip/hip_runtime.h>

#include <sched.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "fedagg_internal.h"

namespace {

constexpr uint64_t kShardAlign = 512;     // elements: every shard row starts 256-B aligned (sharding.SHARD_ALIGN)
constexpr uint64_t kRowAlignBytes = 256;  // row stride of a staged [K, ld] bucket (layout.ROW_ALIGN_BYTES)
constexpr double kHeadroom = 0.85;        // share of free HBM one sub-range may take (multi_device.HBM_HEADROOM)
constexpr int kPackThreadsCap = 32;       // pack workers per GPU past which staging stops scaling
enum { kSlotBucket = 0, kSlotOut = 1, kSlotWs = 2, kSlotC = 3 };  // kSlotC: Scaffold's staged copy of c

int fail(const std::string& msg) {
  fedagg_internal::set_error(msg.c_str());
  return FEDAGG_EINVAL;
}

// "0-3,8,10-11" -> {0,1,2,3,8,10,11}
std::vector<int> parse_cpulist(const std::string& text) {
  std::vector<int> out;
  size_t i = 0;
  while (i < text.size()) {
    size_t j = text.find(',', i);
    if (j == std::string::npos) j = text.size();
    std::string part = text.substr(i, j - i);
    while (!part.empty() && isspace((unsigned char)part.back())) part.pop_back();
    if (!part.empty()) {
      int a = 0, b = 0;
      if (sscanf(part.c_str(), "%d-%d", &a, &b) == 2)
        for (int c = a; c <= b; ++c) out.push_back(c);
      else if (sscanf(part.c_str(), "%d", &a) == 1)
        out.push_back(a);
    }
    i = j + 1;
  }
  return out;
}

std::string read_file(const std::string& path) {
  std::string s;
  if (FILE* f = fopen(path.c_str(), "r")) {
    char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, n);
    fclose(f);
  }
  return s;
}

// NUMA node of a GPU (sysfs numa_node of its PCI function), -1 when unknown
int gpu_numa_node(int device) {
  char bus[64] = {};
  if (fedagg_device_pci_bus_id(device, bus, sizeof(bus)) != FEDAGG_OK) return -1;
  for (char* p = bus; *p; ++p) *p = (char)tolower((unsigned char)*p);
  std::string t = read_file(std::string("/sys/bus/pci/devices/") + bus + "/numa_node");
  int node = -1;
  if (t.empty() || sscanf(t.c_str(), "%d", &node) != 1) return -1;
  return node;
}

std::vector<int> allowed_cpus() {
  std::vector<int> out;
  cpu_set_t set;
  CPU_ZERO(&set);
  if (sched_getaffinity(0, sizeof(set), &set) != 0) return out;
  for (int c = 0; c < CPU_SETSIZE; ++c)
    if (CPU_ISSET(c, &set)) out.push_back(c);
  return out;
}

uint64_t row_ld(uint64_t n, uint64_t esz) {  // multi_device._ld
  const uint64_t per_row = std::max<uint64_t>(1, kRowAlignBytes / esz);
  return std::max(per_row, (n + per_row - 1) / per_row * per_row);
}

struct Shard {
  int device = 0;
  fedagg_session* s = nullptr;
  int numa_node = -1;
  int threads = 0;
  std::vector<int> cpus;
  uint64_t held[4] = {0, 0, 0, 0};  // bytes of the session buffer slots this engine grew
  // the last call
  uint64_t lo = 0, hi = 0;
  int ranges = 0;
  double stage_s = 0, kernel_fetch_s = 0;
};

}  // namespace

struct fedagg_multi {
  std::vector<Shard> shards;
  uint64_t max_shard_bytes = 0;  // 0: kHeadroom of the device's free HBM
  std::mutex m;                  // one aggregation at a time per engine
};

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int shard_buffer(Shard& sh, int slot, uint64_t bytes, void** d) {
  int rc = fedagg_session_buffer(sh.s, slot, bytes, d);
  if (rc == FEDAGG_OK) sh.held[slot] = std::max(sh.held[slot], bytes);
  return rc;
}

// HBM one sub-range of shard g may take: its free HBM plus the buffers the call reuses
int shard_budget(fedagg_multi* m, Shard& sh, uint64_t* budget) {
  if (m->max_shard_bytes) {
    *budget = m->max_shard_bytes;
    return FEDAGG_OK;
  }
  uint64_t free_b = 0, total_b = 0;
  int rc = fedagg_device_memory(sh.device, &free_b, &total_b);
  if (rc) return rc;
  *budget = (uint64_t)((double)(free_b + sh.held[0] + sh.held[1] + sh.held[2]) * kHeadroom);
  return FEDAGG_OK;
}

// The bucket kernel of rows of In averaged into Out (In == Out but for bf16 rows, fp32 output).
template <class In, class Out>
struct KernelOf;
template <>
struct KernelOf<float, float> {
  static int run(const float* const* rows, const void* w, int K, uint64_t n, const uint64_t* idx, int P, void* ws,
                 void* out, void* stream) {
    return fedagg_fedavg_f32(rows, static_cast<const float*>(w), K, n, idx, P, ws, static_cast<float*>(out), stream);
  }
};
template <>
struct KernelOf<double, double> {
  static int run(const double* const* rows, const void* w, int K, uint64_t n, const uint64_t* idx, int P, void* ws,
                 void* out, void* stream) {
    return fedagg_fedavg_f64(rows, static_cast<const double*>(w), K, n, idx, P, ws, static_cast<double*>(out),
                             stream);
  }
};

template <>
struct KernelOf<uint16_t, uint16_t> {  // fp16 buckets (bit patterns), fp16 weights and output: NumPy's half loops
  static int run(const uint16_t* const* rows, const void* w, int K, uint64_t n, const uint64_t* idx, int P, void* ws,
                 void* out, void* stream) {
    return fedagg_fedavg_f16(rows, static_cast<const uint16_t*>(w), K, n, idx, P, ws, static_cast<uint16_t*>(out),
                             stream);
  }
};

template <>
struct KernelOf<uint16_t, float> {  // bf16 buckets (bit patterns), fp32 weights, product, accumulator and output
  static int run(const uint16_t* const* rows, const void* w, int K, uint64_t n, const uint64_t* idx, int P, void* ws,
                 void* out, void* stream) {
    return fedagg_fedavg_bf16(rows, static_cast<const float*>(w), K, n, idx, P, ws, static_cast<float*>(out), stream);
  }
};

// shard_bounds(M, G): equal, 512-element-multiple chunks; the last shards may get less or nothing
void set_shard_bounds(fedagg_multi* m, uint64_t M) {
  const uint64_t G = m->shards.size();
  uint64_t chunk = (M + G - 1) / G;
  chunk = (chunk + kShardAlign - 1) / kShardAlign * kShardAlign;
  for (uint64_t gi = 0; gi < G; ++gi) {
    m->shards[gi].lo = std::min(M, gi * chunk);
    m->shards[gi].hi = std::min(M, (gi + 1) * chunk);
    m->shards[gi].ranges = 0;
  }
}

// HBM one sub-range of every shard may take, per device.  The shard threads of one device all
// allocate from the same free HBM, so it is read once per distinct device here, before any of them
// starts, and divided by the shards on that device; the numel == 1 workspace comes off before the
// step is computed.  With "max_shard_bytes" set that is every shard's budget.
int device_budgets(fedagg_multi* m, size_t ws_bytes, const std::string& name, std::vector<uint64_t>* budget) {
  const uint64_t G = m->shards.size();
  budget->assign(G, m->max_shard_bytes);
  if (m->max_shard_bytes) return FEDAGG_OK;
  for (uint64_t gi = 0; gi < G; ++gi) {
    if ((*budget)[gi]) continue;  // filled in with an earlier shard of the same device
    const int dev = m->shards[gi].device;
    uint64_t free_b = 0, total_b = 0, held = 0, n_on_dev = 0;
    const int rc = fedagg_device_memory(dev, &free_b, &total_b);
    if (rc) {
      const std::string e = fedagg_last_error();
      fail(name + ": free HBM of device " + std::to_string(dev) + ": " + e);
      return rc;
    }
    for (const Shard& sh : m->shards)
      if (sh.device == dev) {
        ++n_on_dev;
        for (uint64_t h : sh.held) held += h;
      }
    const uint64_t share = (uint64_t)((double)(free_b + held) * kHeadroom) / n_on_dev;
    for (uint64_t gj = gi; gj < G; ++gj)
      if (m->shards[gj].device == dev) (*budget)[gj] = std::max<uint64_t>(1, share - std::min<uint64_t>(share, ws_bytes));
  }
  return FEDAGG_OK;
}

// One shard: its sub-ranges through its GPU, in order.  Rows of In, a result of Out; `budget` is the
// HBM one sub-range may take (0: the shard's own free HBM, read here).
template <class In, class Out>
int run_shard(fedagg_multi* m, Shard& sh, int K, int nseg, const void* const* h_seg, const uint64_t* seg_bytes,
              const void* h_w, const std::vector<uint64_t>& idx, Out* h_out, size_t ws_bytes, uint64_t budget) {
  const uint64_t esz = sizeof(In), osz = sizeof(Out);
  sh.ranges = 0;
  sh.stage_s = sh.kernel_fetch_s = 0;
  if (sh.hi <= sh.lo) return FEDAGG_OK;
  int rc = fedagg_session_activate(sh.s);
  if (rc) return rc;
  if (!budget && (rc = shard_budget(m, sh, &budget))) return rc;
  uint64_t cap = std::max<uint64_t>(kShardAlign, budget / ((uint64_t)K * esz + osz));
  const uint64_t step = std::max(kShardAlign, cap / kShardAlign * kShardAlign);  // multi_device._split
  std::vector<const In*> rows(K);
  std::vector<uint64_t> pw;
  for (uint64_t lo = sh.lo; lo < sh.hi; lo += step) {
    const uint64_t hi = std::min(sh.hi, lo + step), n = hi - lo, ld = row_ld(n, esz);
    const double t0 = now_s();
    void *d_bucket = nullptr, *d_out = nullptr, *d_ws = nullptr;
    if ((rc = shard_buffer(sh, kSlotBucket, (uint64_t)K * ld * esz, &d_bucket))) return rc;
    if ((rc = fedagg_session_stage_range(sh.s, d_bucket, ld * esz, K, nseg, h_seg, seg_bytes, lo * esz, hi * esz)))
      return rc;
    const double t1 = now_s();
    if ((rc = shard_buffer(sh, kSlotOut, row_ld(n, osz) * osz, &d_out))) return rc;
    if ((rc = shard_buffer(sh, kSlotWs, ws_bytes, &d_ws))) return rc;
    pw.clear();
    for (uint64_t i : idx)
      if (i >= lo && i < hi) pw.push_back(i - lo);
    for (int k = 0; k < K; ++k)
      rows[k] = reinterpret_cast<const In*>(static_cast<const char*>(d_bucket) + (uint64_t)k * ld * esz);
    if ((rc = KernelOf<In, Out>::run(rows.data(), h_w, K, n, pw.empty() ? nullptr : pw.data(), (int)pw.size(), d_ws,
                                     d_out, fedagg_session_stream(sh.s))))
      return rc;
    if ((rc = fedagg_session_fetch(sh.s, d_out, h_out + lo, n * osz))) return rc;
    sh.stage_s += t1 - t0;
    sh.kernel_fetch_s += now_s() - t1;
    ++sh.ranges;
  }
  return FEDAGG_OK;
}

// The checked call: M > 0 elements of In per row over the shards, into M elements of Out.
// `per_device`: the budget rule of device_budgets (else every shard thread reads its own free HBM).
template <class In, class Out>
int run_fedavg(fedagg_multi* m, int K, int nseg, const void* const* h_seg, const uint64_t* seg_bytes, const void* h_w,
               const std::vector<uint64_t>& idx, uint64_t M, Out* h_out, const std::string& name, bool per_device) {
  std::lock_guard<std::mutex> g(m->m);
  int caller = -1;
  (void)hipGetDevice(&caller);
  const uint64_t G = m->shards.size();
  set_shard_bounds(m, M);
  const size_t ws_bytes = fedagg_pairwise_ws_bytes(K, std::max(1, (int)idx.size()), 8);
  std::vector<uint64_t> budget(G, 0);
  if (per_device)
    if (const int rc = device_budgets(m, ws_bytes, name, &budget)) {
      if (caller >= 0) (void)hipSetDevice(caller);
      return rc;
    }
  std::vector<int> rcs(G, FEDAGG_OK);
  std::vector<std::string> errs(G);
  std::vector<std::thread> th;
  bool spawned = true;
  try {
    for (uint64_t gi = 0; gi < G; ++gi)
      th.emplace_back([&, gi] {
        rcs[gi] = run_shard<In, Out>(m, m->shards[gi], K, nseg, h_seg, seg_bytes, h_w, idx, h_out, ws_bytes,
                                     budget[gi]);
        if (rcs[gi]) errs[gi] = fedagg_last_error();  // the error text is per thread: carry it back
      });
  } catch (const std::exception& e) {  // no thread for a shard: the started ones finish, the call fails
    spawned = false;
    errs.assign(G, std::string("cannot start a shard thread: ") + e.what());
  }
  for (auto& t : th) t.join();
  if (caller >= 0) (void)hipSetDevice(caller);  // the caller's later work stays on its own device
  if (!spawned) return fail(name + ": " + errs[0]);
  for (uint64_t gi = 0; gi < G; ++gi)
    if (rcs[gi]) {
      char buf[640];
      snprintf(buf, sizeof(buf), "%s: shard %d (device %d): %s", name.c_str(), (int)gi, m->shards[gi].device,
               errs[gi].c_str());
      fedagg_internal::set_error(buf);
      return rcs[gi];
    }
  return FEDAGG_OK;
}

template <class T>
int multi_fedavg(fedagg_multi* m, int K, int nseg, const void* const* h_seg, const uint64_t* seg_bytes,
                 const void* h_w, const uint64_t* h_idx, int P, T* h_out, const char* name) {
  if (!m || K <= 0 || nseg < 0 || (nseg > 0 && (!h_seg || !seg_bytes)) || !h_w || P < 0 || (P > 0 && !h_idx) ||
      !h_out)
    return fail(std::string(name) + ": invalid argument");
  uint64_t row = 0;
  for (int i = 0; i < nseg; ++i) {
    if (seg_bytes[i] % sizeof(T)) return fail(std::string(name) + ": segment not a whole number of elements");
    row += seg_bytes[i];
  }
  const uint64_t M = row / sizeof(T);
  std::vector<uint64_t> idx(h_idx, h_idx + P);
  for (uint64_t i : idx)
    if (i >= M) return fail(std::string(name) + ": numel == 1 index out of range");
  if (M == 0) return FEDAGG_OK;
  return run_fedavg<T, T>(m, K, nseg, h_seg, seg_bytes, h_w, idx, M, h_out, name, false);
}

// ---- Scaffold, one bucket per call (fedagg_multi_scaffold_bucket) ----------------------------

uint64_t kind_bytes(int kind) {  // 0: not one of the four float kinds
  switch (kind) {
    case FEDAGG_F16:
    case FEDAGG_BF16: return 2;
    case FEDAGG_F32: return 4;
    case FEDAGG_F64: return 8;
    default: return 0;
  }
}

struct ScaffoldCall {
  int phase, K, nseg, row_kind, Kc, c_nseg, c_kind;
  const void* const* h_rows;
  const uint64_t* seg_bytes;
  const double* h_w;
  double lr;
  const void* const* h_c;
  const uint64_t* c_seg_bytes;
  std::vector<uint64_t> idx;
  double* h_out;
  size_t ws_bytes;
  uint64_t esz, c_esz;
};

// One shard's sub-ranges of one Scaffold bucket, in order; `budget` is the HBM one sub-range may take.
int run_scaffold_shard(Shard& sh, const ScaffoldCall& a, uint64_t budget, uint64_t* mismatches) {
  sh.ranges = 0;
  sh.stage_s = sh.kernel_fetch_s = 0;
  if (sh.hi <= sh.lo) return FEDAGG_OK;
  int rc = fedagg_session_activate(sh.s);
  if (rc) return rc;
  const uint64_t per_elem = (uint64_t)a.K * a.esz + 8 + (a.phase == 1 ? a.c_esz : 0);
  const uint64_t step = std::max(kShardAlign, budget / per_elem / kShardAlign * kShardAlign);  // multi_device._split
  std::vector<const void*> rows(a.K);
  std::vector<uint64_t> pw;
  for (uint64_t lo = sh.lo; lo < sh.hi; lo += step) {
    const uint64_t hi = std::min(sh.hi, lo + step), n = hi - lo, ld = row_ld(n, a.esz);
    const double t0 = now_s();
    void *d_bucket = nullptr, *d_out = nullptr, *d_ws = nullptr, *d_c = nullptr;
    if ((rc = shard_buffer(sh, kSlotBucket, (uint64_t)a.K * ld * a.esz, &d_bucket))) return rc;
    if ((rc = fedagg_session_stage_range(sh.s, d_bucket, ld * a.esz, a.K, a.nseg, a.h_rows, a.seg_bytes, lo * a.esz,
                                         hi * a.esz)))
      return rc;
    if (a.phase == 1) {
      const uint64_t ldc = row_ld(n, a.c_esz) * a.c_esz;
      if ((rc = shard_buffer(sh, kSlotC, ldc, &d_c))) return rc;
      if (a.Kc == a.K) {  // copy 0 staged, the others compared with it on the pack workers
        uint64_t bad = 0;
        if ((rc = fedagg_session_stage_check(sh.s, d_c, a.K, a.c_nseg, a.h_c, a.c_seg_bytes, lo * a.c_esz,
                                             hi * a.c_esz, a.c_kind, &bad)))
          return rc;
        *mismatches += bad;
      } else if ((rc = fedagg_session_stage_range(sh.s, d_c, ldc, 1, a.c_nseg, a.h_c, a.c_seg_bytes, lo * a.c_esz,
                                                  hi * a.c_esz))) {
        return rc;
      }
    }
    const double t1 = now_s();
    if ((rc = shard_buffer(sh, kSlotOut, row_ld(n, 8) * 8, &d_out))) return rc;
    if ((rc = shard_buffer(sh, kSlotWs, a.ws_bytes, &d_ws))) return rc;
    pw.clear();
    for (uint64_t i : a.idx)
      if (i >= lo && i < hi) pw.push_back(i - lo);
    for (int k = 0; k < a.K; ++k) rows[k] = static_cast<const char*>(d_bucket) + (uint64_t)k * ld * a.esz;
    if ((rc = fedagg_scaffold_bucket(rows.data(), a.row_kind, a.h_w, a.K, n, a.phase, d_c, a.c_kind, a.lr,
                                     pw.empty() ? nullptr : pw.data(), (int)pw.size(), d_ws,
                                     static_cast<double*>(d_out), fedagg_session_stream(sh.s))))
      return rc;
    if ((rc = fedagg_session_fetch(sh.s, d_out, a.h_out + lo, n * 8))) return rc;
    sh.stage_s += t1 - t0;
    sh.kernel_fetch_s += now_s() - t1;
    ++sh.ranges;
  }
  return FEDAGG_OK;
}

}  // namespace

extern "C" {

fedagg_multi* fedagg_multi_create(int ndev, const int* devs, int pack_threads) {
  if (ndev <= 0 || !devs || pack_threads < 0 || pack_threads > 256) {
    fail("fedagg_multi_create: need ndev >= 1 device indices and 0 <= pack_threads <= 256");
    return nullptr;
  }
  int caller = -1;
  (void)hipGetDevice(&caller);
  auto* m = new (std::nothrow) fedagg_multi();
  if (!m) {
    fail("fedagg_multi_create: out of host memory");
    return nullptr;
  }
  const std::vector<int> allowed = allowed_cpus();
  const int per = pack_threads ? pack_threads
                               : std::max(2, std::min(kPackThreadsCap, (int)allowed.size() / ndev));
  for (int g = 0; g < ndev; ++g) {
    Shard sh;
    sh.device = devs[g];
    sh.s = fedagg_session_create(devs[g]);  // a private session: its buffers, ring and workers
    if (!sh.s) {
      std::string e = fedagg_last_error();
      for (auto& o : m->shards) fedagg_session_destroy(o.s);
      delete m;
      if (caller >= 0) (void)hipSetDevice(caller);
      fail("fedagg_multi_create: device " + std::to_string(devs[g]) + ": " + e);
      return nullptr;
    }
    sh.threads = per;
    sh.numa_node = gpu_numa_node(devs[g]);
    if (sh.numa_node >= 0) {  // the allowed CPUs of the GPU's node (multi_device.node_cpus)
      std::vector<int> node = parse_cpulist(
          read_file("/sys/devices/system/node/node" + std::to_string(sh.numa_node) + "/cpulist"));
      for (int c : node)
        if (std::find(allowed.begin(), allowed.end(), c) != allowed.end()) sh.cpus.push_back(c);
    }
    int rc = fedagg_session_set(sh.s, "threads", per);
    if (!rc) rc = fedagg_session_affinity(sh.s, sh.cpus.data(), (int)sh.cpus.size());
    if (rc) {
      std::string e = fedagg_last_error();
      fedagg_session_destroy(sh.s);
      for (auto& o : m->shards) fedagg_session_destroy(o.s);
      delete m;
      if (caller >= 0) (void)hipSetDevice(caller);
      fail("fedagg_multi_create: placement of device " + std::to_string(devs[g]) + ": " + e);
      return nullptr;
    }
    m->shards.push_back(std::move(sh));
  }
  if (caller >= 0) (void)hipSetDevice(caller);
  return m;
}

void fedagg_multi_destroy(fedagg_multi* m) {
  if (!m) return;
  int caller = -1;
  (void)hipGetDevice(&caller);
  {
    std::lock_guard<std::mutex> g(m->m);
    for (auto& sh : m->shards) fedagg_session_destroy(sh.s);
  }
  if (caller >= 0) (void)hipSetDevice(caller);
  delete m;
}

int fedagg_multi_set(fedagg_multi* m, const char* key, long long value) {
  if (!m || !key) return fail("fedagg_multi_set: invalid argument");
  std::lock_guard<std::mutex> g(m->m);
  if (!strcmp(key, "max_shard_bytes") && value >= 0) {
    m->max_shard_bytes = (uint64_t)value;
    return FEDAGG_OK;
  }
  if (!strcmp(key, "threads") && value >= 1 && value <= 256) {
    for (auto& sh : m->shards) {
      int rc = fedagg_session_set(sh.s, "threads", value);
      if (rc) return rc;
      sh.threads = (int)value;
    }
    return FEDAGG_OK;
  }
  return fail("fedagg_multi_set: unknown key or bad value");
}

int fedagg_multi_fedavg_f32(fedagg_multi* m, int K, int nseg, const void* const* h_seg, const uint64_t* seg_bytes,
                            const float* h_w, const uint64_t* h_idx, int P, float* h_out) {
  return multi_fedavg<float>(m, K, nseg, h_seg, seg_bytes, h_w, h_idx, P, h_out, "fedagg_multi_fedavg_f32");
}

int fedagg_multi_fedavg_f64(fedagg_multi* m, int K, int nseg, const void* const* h_seg, const uint64_t* seg_bytes,
                            const double* h_w, const uint64_t* h_idx, int P, double* h_out) {
  return multi_fedavg<double>(m, K, nseg, h_seg, seg_bytes, h_w, h_idx, P, h_out, "fedagg_multi_fedavg_f64");
}

int fedagg_multi_fedavg_f16(fedagg_multi* m, int K, int nseg, const void* const* h_seg, const uint64_t* seg_bytes,
                            const uint16_t* h_w, const uint64_t* h_idx, int P, uint16_t* h_out) {
  return multi_fedavg<uint16_t>(m, K, nseg, h_seg, seg_bytes, h_w, h_idx, P, h_out, "fedagg_multi_fedavg_f16");
}

int fedagg_multi_fedavg_bf16(fedagg_multi* m, int K, int nseg, const void* const* h_seg, const uint64_t* seg_bytes,
                             const float* h_w, const uint64_t* h_idx, int P, float* h_out) {
  const std::string name = "fedagg_multi_fedavg_bf16";
  // every argument check comes before the first HIP call, the engine last
  if (K <= 0) return fail(name + ": K must be > 0");
  if (!h_w || nseg < 0 || (nseg > 0 && (!h_seg || !seg_bytes)) || P < 0 || (P > 0 && !h_idx))
    return fail(name + ": invalid argument");
  uint64_t row = 0;
  for (int i = 0; i < nseg; ++i) {
    if (seg_bytes[i] % 2) return fail(name + ": segment not a whole number of elements");
    row += seg_bytes[i];
  }
  const uint64_t M = row / 2;
  std::vector<uint64_t> idx(h_idx, h_idx + P);
  for (uint64_t i : idx)
    if (i >= M) return fail(name + ": numel == 1 index out of range");
  if (!h_out) return fail(name + ": NULL h_out");
  if (!m) return fail(name + ": NULL engine");
  if (M == 0) return FEDAGG_OK;
  return run_fedavg<uint16_t, float>(m, K, nseg, h_seg, seg_bytes, h_w, idx, M, h_out, name, true);
}

int fedagg_multi_scaffold_bucket(fedagg_multi* m, int phase, int K, int nseg, const void* const* h_rows,
                                 const uint64_t* seg_bytes, int row_kind, const double* h_w, double lr, int Kc,
                                 int c_nseg, const void* const* h_c, const uint64_t* c_seg_bytes, int c_kind,
                                 const uint64_t* h_idx, int P, double* h_out, uint64_t* mismatches) {
  const std::string name = "fedagg_multi_scaffold_bucket";
  // every argument check comes before the first HIP call
  if (K <= 0) return fail(name + ": K must be > 0");
  if (phase != 0 && phase != 1) return fail(name + ": phase must be 0 or 1");
  ScaffoldCall a{};
  a.esz = kind_bytes(row_kind);
  if (!a.esz) return fail(name + ": unknown row kind");
  if (nseg < 0 || (nseg > 0 && (!h_rows || !seg_bytes)) || !h_w || P < 0 || (P > 0 && !h_idx))
    return fail(name + ": invalid argument");
  uint64_t row = 0;
  for (int i = 0; i < nseg; ++i) {
    if (seg_bytes[i] % a.esz) return fail(name + ": segment not a whole number of elements");
    row += seg_bytes[i];
  }
  const uint64_t M = row / a.esz;
  if (phase == 1) {
    a.c_esz = kind_bytes(c_kind);
    if (!a.c_esz) return fail(name + ": unknown c kind");
    if ((row_kind == FEDAGG_F32 || row_kind == FEDAGG_F64) && c_kind != row_kind)
      return fail(name + ": c kind must equal the kind of f32 / f64 rows");
    if (Kc != 1 && Kc != K) return fail(name + ": Kc must be 1 or K");
    if (c_nseg < 0 || (c_nseg > 0 && (!h_c || !c_seg_bytes))) return fail(name + ": invalid c argument");
    uint64_t c_row = 0;
    for (int i = 0; i < c_nseg; ++i) {
      if (c_seg_bytes[i] % a.c_esz) return fail(name + ": c segment not a whole number of elements");
      c_row += c_seg_bytes[i];
    }
    if (c_row / a.c_esz != M) return fail(name + ": a c row does not total M elements");
    for (int k = 0; k < Kc; ++k)
      for (int i = 0; i < c_nseg; ++i)
        if (!h_c[(size_t)k * c_nseg + i] && c_seg_bytes[i]) return fail(name + ": NULL c segment");
    if (Kc == K && !mismatches) return fail(name + ": NULL mismatches with Kc == K");
  }
  a.idx.assign(h_idx, h_idx + P);
  for (uint64_t i : a.idx)
    if (i >= M) return fail(name + ": numel == 1 index out of range");
  if (!h_out) return fail(name + ": NULL h_out");
  if (!m) return fail(name + ": NULL engine");
  if (phase == 1 && mismatches) *mismatches = 0;
  if (M == 0) return FEDAGG_OK;
  a.phase = phase, a.K = K, a.nseg = nseg, a.row_kind = row_kind;
  a.Kc = Kc, a.c_nseg = c_nseg, a.c_kind = phase == 1 ? c_kind : FEDAGG_F64;
  a.h_rows = h_rows, a.seg_bytes = seg_bytes, a.h_w = h_w, a.lr = lr;
  a.h_c = h_c, a.c_seg_bytes = c_seg_bytes, a.h_out = h_out;
  a.ws_bytes = fedagg_pairwise_ws_bytes(K, std::max(1, P), 8);
  std::lock_guard<std::mutex> g(m->m);
  int caller = -1;
  (void)hipGetDevice(&caller);
  const uint64_t G = m->shards.size();
  set_shard_bounds(m, M);
  std::vector<uint64_t> budget;
  if (const int rc = device_budgets(m, a.ws_bytes, name, &budget)) {
    if (caller >= 0) (void)hipSetDevice(caller);
    return rc;
  }
  std::vector<int> rcs(G, FEDAGG_OK);
  std::vector<uint64_t> bad(G, 0);
  std::vector<std::string> errs(G);
  std::vector<std::thread> th;
  bool spawned = true;
  try {
    for (uint64_t gi = 0; gi < G; ++gi)
      th.emplace_back([&, gi] {
        rcs[gi] = run_scaffold_shard(m->shards[gi], a, budget[gi], &bad[gi]);
        if (rcs[gi]) errs[gi] = fedagg_last_error();  // the error text is per thread: carry it back
      });
  } catch (const std::exception& e) {  // no thread for a shard: the started ones finish, the call fails
    spawned = false;
    errs.assign(G, std::string("cannot start a shard thread: ") + e.what());
  }
  for (auto& t : th) t.join();
  if (caller >= 0) (void)hipSetDevice(caller);  // the caller's later work stays on its own device
  if (!spawned) return fail(name + ": " + errs[0]);
  for (uint64_t gi = 0; gi < G; ++gi)
    if (rcs[gi]) {
      char buf[640];
      snprintf(buf, sizeof(buf), "%s: shard %d (device %d): %s", name.c_str(), (int)gi, m->shards[gi].device,
               errs[gi].c_str());
      fedagg_internal::set_error(buf);
      return rcs[gi];
    }
  if (phase == 1 && Kc == K)
    for (uint64_t gi = 0; gi < G; ++gi) *mismatches += bad[gi];
  return FEDAGG_OK;
}

int fedagg_multi_shard_info(fedagg_multi* m, int g, int* device, int* numa_node, int* threads, int* ncpus,
                            uint64_t* lo, uint64_t* hi, int* ranges) {
  if (!m || g < 0 || g >= (int)m->shards.size()) return fail("fedagg_multi_shard_info: no such shard");
  std::lock_guard<std::mutex> lk(m->m);
  const Shard& sh = m->shards[g];
  if (device) *device = sh.device;
  if (numa_node) *numa_node = sh.numa_node;
  if (threads) *threads = sh.threads;
  if (ncpus) *ncpus = (int)sh.cpus.size();
  if (lo) *lo = sh.lo;
  if (hi) *hi = sh.hi;
  if (ranges) *ranges = sh.ranges;
  return FEDAGG_OK;
}

}  // extern "C"
