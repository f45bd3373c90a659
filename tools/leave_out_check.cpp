// leave_out_check.cpp -- the index check of gmb_leave_out (gumbi_amd/csrc/leave_out.hpp: leave_out_check_indices, the very function
// engine.hip calls before anything is launched) as a stand-alone program for the sanitizers.  No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/leave_out_check.cpp -o /tmp/leave_out_check
//   /tmp/leave_out_check
//
// Driven: accepted index sets (one row, all rows, scrambled), m out of [1, N], a null pointer, an index below 0, at N and far beyond
// it (nothing indexed with it), a duplicate at the front, at the back and of the last row -- with the offending position.
// One line per failure; exit status 0 when all agree (tests/test_leave_out_cpu.py builds and runs it without the sanitizers).
#include <cstdio>
#include <numeric>
#include <utility>
#include <vector>

#define LEAVE_OUT_HOST_ONLY  // the kernels of the header stay out
#include "../gumbi_amd/csrc/leave_out.hpp"

using namespace gmb;

static int failures = 0;

static void expect(const char* name, const std::vector<int64_t>& idx, int64_t m, int64_t N, int want, int64_t want_pos) {
  int64_t pos = -7;
  const int got = leave_out_check_indices(idx.empty() ? nullptr : idx.data(), m, N, &pos);
  if (got != want || pos != want_pos) {
    std::printf("FAIL %s: status %d at %lld, expected %d at %lld\n", name, got, (long long)pos, want, (long long)want_pos);
    ++failures;
  }
}

int main() {
  const int64_t N = 700;
  std::vector<int64_t> all((size_t)N);
  std::iota(all.begin(), all.end(), (int64_t)0);
  expect("all rows", all, N, N, 0, -1);
  expect("one row", {699}, 1, N, 0, -1);
  expect("first row", {0}, 1, N, 0, -1);
  std::vector<int64_t> scrambled = all;
  for (size_t i = 0; i + 1 < scrambled.size(); i += 2) std::swap(scrambled[i], scrambled[i + 1]);
  expect("scrambled", scrambled, N, N, 0, -1);
  expect("a prefix of a longer array", all, 37, N, 0, -1);

  expect("m = 0", {1, 2}, 0, N, 1, -1);
  expect("m < 0", {1, 2}, -3, N, 1, -1);
  std::vector<int64_t> longer((size_t)N + 1, 0);
  expect("m > N", longer, N + 1, N, 1, -1);
  expect("null idx", {}, 3, N, 1, -1);
  expect("no rows at all", {0}, 1, 0, 1, -1);

  expect("index = N", {5, N, 6}, 3, N, 2, 1);
  expect("index < 0", {-1, 4}, 2, N, 2, 0);
  expect("index far out", {4, 3, (int64_t)1 << 62}, 3, N, 2, 2);
  expect("index INT64_MIN", {4, INT64_MIN}, 2, N, 2, 1);

  expect("duplicate at the front", {9, 9, 3}, 3, N, 3, 1);
  expect("duplicate at the back", {1, 2, 3, 4, 1}, 5, N, 3, 4);
  expect("duplicate of the last row", {699, 0, 699}, 3, N, 3, 2);
  expect("out of range before the duplicate", {9, 700, 9}, 3, N, 2, 1);

  // the position pointer is optional
  const int64_t two[2] = {3, 3};
  if (leave_out_check_indices(two, 2, N, nullptr) != 3) {
    std::printf("FAIL null position pointer\n");
    ++failures;
  }
  std::printf("leave_out_check: %d failure%s\n", failures, failures == 1 ? "" : "s");
  return failures ? 1 : 0;
}
