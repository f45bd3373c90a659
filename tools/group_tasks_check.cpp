// group_tasks_check.cpp -- the host-side arithmetic of gmb_predict_groups (gumbi_amd/csrc/group_tasks.hpp: group_check_offsets and
// group_build_tasks, the very functions engine.hip calls before anything is launched) as a stand-alone program for the
// sanitizers.  No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/group_tasks_check.cpp -o /tmp/group_tasks_check
//   /tmp/group_tasks_check
//
// Driven: accepted offsets (one group, many, the engine's chunk and small ones), every refusal with the offending group (null, G < 1,
// a first offset that is not 0, an empty group at the front, in the middle and at the end, offsets that run backwards, a last
// offset that is not M), and for the task lists: every point in exactly one task, counts in [1, chunk], ascending group and then
// ascending first point, first_task consistent -- for group sizes 1, chunk, chunk + 1, 2 chunk + 1 and a mixed list.
// One line per failure; exit status 0 when all agree (tests/test_group_average_cpu.py builds and runs it without the sanitizers).
#include <cstdio>
#include <vector>

#include "../gumbi_amd/csrc/group_tasks.hpp"

using namespace gmb;

static int failures = 0;

static void expect(const char* name, const std::vector<int64_t>& off, int64_t G, int64_t M, int want, int64_t want_pos) {
  int64_t pos = -7;
  const int got = group_check_offsets(off.empty() ? nullptr : off.data(), G, M, &pos);
  if (got != want || pos != want_pos) {
    std::printf("FAIL %s: status %d at %lld, expected %d at %lld\n", name, got, (long long)pos, want, (long long)want_pos);
    ++failures;
  }
}

static std::vector<int64_t> offsets_of(const std::vector<int64_t>& sizes) {
  std::vector<int64_t> off(1, 0);
  for (int64_t n : sizes) off.push_back(off.back() + n);
  return off;
}

static void check_tasks(const char* name, const std::vector<int64_t>& sizes, int64_t chunk) {
  const std::vector<int64_t> off = offsets_of(sizes);
  const int64_t G = (int64_t)sizes.size(), M = off.back();
  auto bad = [&](const char* what, long long at) {
    std::printf("FAIL %s (chunk %lld): %s at %lld\n", name, (long long)chunk, what, at);
    ++failures;
  };
  if (group_check_offsets(off.data(), G, M, nullptr) != 0) return bad("offsets refused", -1);
  std::vector<int64_t> tasks, first;
  const int64_t n = group_build_tasks(off.data(), G, chunk, &tasks, &first);
  if (n != group_task_count(off.data(), G, chunk) || (int64_t)tasks.size() != 3 * n) return bad("task count", n);
  if ((int64_t)first.size() != G + 1 || first[0] != 0 || first[(size_t)G] != n) return bad("first_task ends", n);
  std::vector<int> seen((size_t)M, 0);
  for (int64_t t = 0; t < n; ++t) {
    const int64_t g = tasks[(size_t)(3 * t)], m0 = tasks[(size_t)(3 * t + 1)], cnt = tasks[(size_t)(3 * t + 2)];
    if (g < 0 || g >= G) return bad("group out of range", t);
    if (cnt < 1 || cnt > chunk) return bad("count outside [1, chunk]", t);
    if (m0 < off[(size_t)g] || m0 + cnt > off[(size_t)g + 1]) return bad("task leaves its group", t);
    if (t < first[(size_t)g] || t >= first[(size_t)g + 1]) return bad("first_task disagrees", t);
    if (t > 0) {
      const int64_t gp = tasks[(size_t)(3 * t - 3)], mp = tasks[(size_t)(3 * t - 2)];
      if (g < gp || (g == gp && m0 <= mp)) return bad("order", t);
    }
    for (int64_t m = m0; m < m0 + cnt; ++m) ++seen[(size_t)m];
  }
  for (int64_t m = 0; m < M; ++m)
    if (seen[(size_t)m] != 1) return bad("a point is not in exactly one task", m);
  // a group of n points has ceil(n / chunk) tasks, all full but the last
  for (int64_t g = 0; g < G; ++g)
    if (first[(size_t)g + 1] - first[(size_t)g] != (sizes[(size_t)g] + chunk - 1) / chunk) return bad("tasks per group", g);
}

int main() {
  expect("one group", {0, 5}, 1, 5, 0, -1);
  expect("three groups", {0, 1, 4, 9}, 3, 9, 0, -1);
  expect("a prefix of a longer array", {0, 2, 4, 6, 8}, 2, 4, 0, -1);

  expect("null offsets", {}, 2, 4, 1, -1);
  expect("G = 0", {0}, 0, 0, 1, -1);
  expect("G < 0", {0, 3}, -1, 3, 1, -1);
  expect("first offset not 0", {1, 3, 5}, 2, 5, 2, -1);
  expect("empty group at the front", {0, 0, 5}, 2, 5, 3, 0);
  expect("empty group in the middle", {0, 2, 2, 5}, 3, 5, 3, 1);
  expect("empty group at the end", {0, 2, 5, 5}, 3, 5, 3, 2);
  expect("offsets run backwards", {0, 4, 3, 9}, 3, 9, 3, 1);
  expect("last offset short of M", {0, 2, 5}, 2, 6, 4, -1);
  expect("last offset beyond M", {0, 2, 7}, 2, 6, 4, -1);
  expect("empty group before a wrong end", {0, 2, 2, 7}, 3, 6, 3, 1);
  if (group_check_offsets(std::vector<int64_t>{0, 0}.data(), 1, 0, nullptr) != 3) {  // the position pointer is optional
    std::printf("FAIL null position pointer\n");
    ++failures;
  }

  for (int64_t chunk : {(int64_t)1, (int64_t)4, (int64_t)128, GROUP_CHUNK}) {
    check_tasks("one point", {1}, chunk);
    check_tasks("a chunk", {chunk}, chunk);
    check_tasks("a chunk and a point", {chunk + 1}, chunk);
    check_tasks("two chunks and a point", {2 * chunk + 1}, chunk);
    check_tasks("mixed", {1, 2, 127, 128, 129, 2 * chunk + 1, 300, 64, 5, 131, chunk, chunk + 1, 1}, chunk);
  }
  std::printf("group_tasks_check: %d failure%s\n", failures, failures == 1 ? "" : "s");
  return failures ? 1 : 0;
}
