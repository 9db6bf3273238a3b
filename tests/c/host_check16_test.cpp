// The 16-bit kinds of the host value check (substrafl_amd/csrc/host_pool.h: count_mismatch_range /
// check_rows with kHalfF16 / kHalfBF16), the compare fedagg_session_stage_check runs on the pack
// workers for fp16 and bf16 copies of Scaffold's server control variate (scaffold.py:193-196,
// np.testing.assert_array_equal: +0 == -0, NaN == NaN).  Every expected count is the number of
// differences planted.  Stand-alone: g++ -std=c++17 -pthread -Isubstrafl_amd/csrc, plain or with
// -fsanitize=address,undefined (tests/test_host_check16.py); every segment is its own allocation,
// so a read past a segment's end is an AddressSanitizer error.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "host_pool.h"

using fedagg_host::check_rows;
using fedagg_host::kHalfBF16;
using fedagg_host::kHalfF16;
using fedagg_host::Pool;

namespace {

int failures = 0;

void expect(uint64_t got, uint64_t want, const char* what, int half) {
  if (got == want) return;
  fprintf(stderr, "%s (%s): got %llu, want %llu\n", what, half == kHalfF16 ? "f16" : half == kHalfBF16 ? "bf16" : "-",
          (unsigned long long)got, (unsigned long long)want);
  ++failures;
}

// K copies of one row of 2-byte elements cut into uneven segments, each segment its own allocation
struct Rows {
  std::vector<uint64_t> numel, bytes, start;  // per segment; start = first flat element
  int K;
  uint64_t M = 0;
  std::vector<std::unique_ptr<uint16_t[]>> mem;
  std::vector<const void*> seg;  // [k * nseg + i]
  Rows(int K_, std::vector<uint64_t> numel_) : numel(std::move(numel_)), K(K_) {
    for (uint64_t n : numel) {
      start.push_back(M);
      bytes.push_back(n * 2);
      M += n;
    }
    uint32_t s = 12345u;
    std::vector<uint16_t> base(M);
    for (auto& v : base) {
      s = s * 1664525u + 1013904223u;
      v = (uint16_t)((s >> 16) & 0x3BFF);  // finite, positive, the same value in both kinds' terms
    }
    for (int k = 0; k < K; ++k)
      for (size_t i = 0; i < numel.size(); ++i) {
        mem.emplace_back(new uint16_t[numel[i] ? numel[i] : 1]);
        memcpy(mem.back().get(), base.data() + start[i], numel[i] * 2);
        seg.push_back(mem.back().get());
      }
  }
  int nseg() const { return (int)numel.size(); }
  uint16_t& at(int k, uint64_t e) {
    size_t i = 0;
    while (i + 1 < numel.size() && e >= start[i] + numel[i]) ++i;
    return mem[(size_t)k * numel.size() + i][e - start[i]];
  }
  void all(uint64_t e, uint16_t v) {
    for (int k = 0; k < K; ++k) at(k, e) = v;
  }
  void reset() {
    for (int k = 1; k < K; ++k)
      for (size_t i = 0; i < numel.size(); ++i)
        memcpy(mem[(size_t)k * numel.size() + i].get(), mem[i].get(), numel[i] * 2);
  }
  uint64_t check(Pool& pool, int half, uint64_t e_lo, uint64_t e_hi) {
    return check_rows(pool, seg.data(), bytes.data(), nseg(), K, e_lo * 2, (e_hi - e_lo) * 2, 2, half);
  }
  uint64_t check(Pool& pool, int half) { return check(pool, half, 0, M); }
};

void run_kind(Pool& pool, int half) {
  const uint16_t inf = half == kHalfF16 ? 0x7C00 : 0x7F80;
  const uint16_t qnan = half == kHalfF16 ? 0x7E00 : 0x7FC0;
  // 601 041 elements: longer than one 1 MiB piece (524 288 elements), pieces cutting through a segment
  Rows r(5, {3, 1000, 1, 600000, 37});
  const uint64_t M = r.M;
  expect(r.check(pool, half), 0, "identical copies", half);

  r.at(0, 5) = 0x0000, r.at(1, 5) = 0x8000, r.at(2, 5) = 0x8000, r.at(3, 5) = 0x0000, r.at(4, 5) = 0x8000;
  expect(r.check(pool, half), 0, "+0 / -0", half);
  r.all(7, 0x8000), r.at(1, 7) = 0x0000;
  expect(r.check(pool, half), 0, "-0 / +0", half);

  r.at(0, 9) = qnan;
  for (int k = 1; k < 5; ++k) r.at(k, 9) = (uint16_t)((k & 1 ? 0x8000 : 0) | (inf + k));  // sign and payload vary
  expect(r.check(pool, half), 0, "NaN of another sign and payload", half);

  r.at(0, 11) = inf, r.at(1, 11) = qnan, r.at(2, 11) = (uint16_t)(inf + 1), r.at(3, 11) = inf, r.at(4, 11) = inf;
  expect(r.check(pool, half), 2, "NaN against inf", half);
  r.at(0, 11) = qnan, r.at(1, 11) = inf, r.at(2, 11) = (uint16_t)(0x8000 | inf), r.at(3, 11) = qnan, r.at(4, 11) = qnan;
  expect(r.check(pool, half), 2, "inf against NaN", half);
  r.all(11, inf), r.at(1, 11) = (uint16_t)(0x8000 | inf);
  expect(r.check(pool, half), 1, "+inf against -inf", half);
  r.reset();

  // the pair that tells the kinds apart: two NaNs as fp16, two finite values as bf16
  r.all(500, 0x7E00), r.at(3, 500) = 0x7E01;
  expect(r.check(pool, half), half == kHalfF16 ? 0 : 1, "0x7E00 / 0x7E01", half);
  r.all(500, 0x7F90), r.at(3, 500) = 0x7F91;
  expect(r.check(pool, half), 0, "0x7F90 / 0x7F91 (NaN in both kinds)", half);
  r.all(500, 0x7C00), r.at(3, 500) = 0x7C01;  // fp16: inf against NaN; bf16: two finite values
  expect(r.check(pool, half), 1, "0x7C00 / 0x7C01", half);
  r.reset();

  r.at(2, M - 1) ^= 0x0001;
  expect(r.check(pool, half), 1, "the last element", half);
  // both sides of a segment boundary (segment 1 ends at 1003, the one-element segment 2 at 1004)
  r.at(1, 1002) ^= 0x0010, r.at(1, 1003) ^= 0x0010, r.at(4, 1004) ^= 0x0010;
  expect(r.check(pool, half), 4, "across segment boundaries", half);
  // around the 1 MiB piece boundary of the whole row, and of a window that starts mid-segment
  r.at(3, 524287) ^= 0x0100, r.at(3, 524288) ^= 0x0100;
  expect(r.check(pool, half), 6, "across the piece boundary", half);
  expect(r.check(pool, half, 1003, M), 5, "window from a segment boundary", half);
  expect(r.check(pool, half, 1500, M), 3, "window from the middle of segment 3", half);
  expect(r.check(pool, half, 1003, M - 1), 4, "window without the last element", half);
  expect(r.check(pool, half, 1004, 524288), 2, "window ending at the piece boundary", half);
  expect(r.check(pool, half, 1500, 2012), 0, "a clean window inside segment 3", half);
  expect(r.check(pool, half, 524288, 524289), 1, "a one-element window", half);
  expect(r.check(pool, half, 700, 700), 0, "an empty window", half);
  r.at(1, 1500 + 524288) ^= 0x0001;  // second piece of the window [1500, M)
  expect(r.check(pool, half, 1500, M), 4, "window longer than one piece", half);
  r.reset();

  // every copy differs in one place: K = 5 counts K - 1
  for (int k = 1; k < 5; ++k) r.at(k, (uint64_t)k * 100003) ^= 0x0002;
  expect(r.check(pool, half), 4, "one difference per copy", half);
  // a difference in row 0 is a difference against every copy
  r.reset();
  r.at(0, 2) ^= 0x0004;
  expect(r.check(pool, half), 4, "row 0 differs from every copy", half);

  Rows one(1, {3, 1000, 1, 37});
  one.at(0, 2) = qnan;
  expect(one.check(pool, half), 0, "K = 1", half);
}

template <class T, class U>
void run_wide(Pool& pool, int esz) {
  const uint64_t n[2] = {1025, 300001};  // 8-byte rows longer than one piece too
  const int K = 3;
  std::vector<std::vector<T>> mem;
  std::vector<const void*> seg;
  std::vector<uint64_t> bytes = {n[0] * sizeof(T), n[1] * sizeof(T)};
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < 2; ++i) {
      mem.emplace_back(n[i]);
      for (uint64_t e = 0; e < n[i]; ++e) mem.back()[e] = (T)(0.25 * (double)(e % 977) - 3.0);
    }
  for (auto& v : mem) seg.push_back(v.data());
  const uint64_t row = bytes[0] + bytes[1];
  auto check = [&] { return check_rows(pool, seg.data(), bytes.data(), 2, K, 0, row, esz); };
  expect(check(), 0, "wide: identical", 0);
  mem[0][12] = (T)0.0, mem[2][12] = (T)-0.0;
  expect(check(), 0, "wide: +0 / -0", 0);
  const U nan_a = sizeof(T) == 4 ? (U)0x7FC00000u : (U)0x7FF8000000000000ull;
  const U nan_b = sizeof(T) == 4 ? (U)0xFFC00001u : (U)0xFFF8000000000001ull;
  memcpy(&mem[1][5], &nan_a, sizeof(T));      // row 0, segment 1
  memcpy(&mem[3][5], &nan_b, sizeof(T));      // row 1
  memcpy(&mem[5][5], &nan_a, sizeof(T));      // row 2
  expect(check(), 0, "wide: NaN payloads", 0);
  mem[2][1024] += (T)1.0;
  mem[5][300000] += (T)1.0;
  mem[3][0] += (T)1.0;
  expect(check(), 3, "wide: three planted differences", 0);
  expect(check_rows(pool, seg.data(), bytes.data(), 2, K, bytes[0], bytes[1], esz), 2, "wide: second segment only", 0);
}

}  // namespace

int main() {
  Pool pool(4);
  run_kind(pool, kHalfF16);
  run_kind(pool, kHalfBF16);
  run_wide<float, uint32_t>(pool, 4);
  run_wide<double, uint64_t>(pool, 8);
  if (failures) {
    fprintf(stderr, "host_check16_test: %d failures\n", failures);
    return 1;
  }
  printf("host_check16_test: ok\n");
  return 0;
}
