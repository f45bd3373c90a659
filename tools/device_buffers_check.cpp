// device_buffers_check.cpp -- the engine's buffer ownership (gumbi_amd/csrc/device_buffers.hpp: the very header engine.hip owns its
// device memory with) driven over a HOST allocator, as a stand-alone program for the sanitizers.  No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/device_buffers_check.cpp -o /tmp/device_buffers_check
//   /tmp/device_buffers_check
//
// The two allocator hooks are malloc / free with a live set of their own, so the program itself says "double free", "free of
// unknown block" and "N blocks live at exit", and the allocator can be told to fail its k-th allocation from now.  Driven:
//   * reserve: no-op when large enough, grow, and after stale() (the old block goes at THAT reserve, not before);
//   * renew, drop, adopt, a ScopedBuf abandoned by an early return;
//   * a row group's reserve whose 1st ... last member allocation fails: no rows claimed, nothing leaked, the retry succeeds;
//   * counted against uncounted blocks in resident / peak bytes;
//   * release_all leaves the allocator empty.
// One line per case; exit status 0 when all agree (tests/test_device_buffers_cpu.py builds and runs it without the sanitizers).
#include <cstdio>
#include <cstdlib>
#include <set>

#define GMB_DEVBUF_OWN_HOOKS  // the allocator is this file's
#include "../gumbi_amd/csrc/device_buffers.hpp"

using namespace gmb;

static int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::printf("FAIL %s: ", #cond);   \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
      ++failures;                        \
    }                                    \
  } while (0)

// ---- the host allocator behind the hooks ---------------------------------------------------------------------------------
static std::set<void*> live_blocks;
static int allocs_seen = 0, frees_seen = 0;
static int fail_in = 0;  // > 0: the fail_in-th allocation from now fails
static int owner_told = 0;

const char* gmb::devbuf_alloc(void** p, size_t bytes) {
  if (fail_in > 0 && --fail_in == 0) return "told to fail";
  *p = std::malloc(bytes);
  CHECK(*p != nullptr && bytes > 0, "malloc of %zu bytes", bytes);
  live_blocks.insert(*p);
  ++allocs_seen;
  return nullptr;
}

// what the pool tells its owner about a refused allocation (the engine writes its error text here)
static int refused(void* owner, size_t bytes, const char* why) {
  CHECK(bytes > 0 && why != nullptr, "a refusal names its size and its reason");
  ++*static_cast<int*>(owner);
  return -7;
}

void gmb::devbuf_free(void* p) {
  ++frees_seen;
  if (!live_blocks.count(p)) {
    CHECK(false, "double free or free of unknown block %p", p);
    return;
  }
  live_blocks.erase(p);
  std::free(p);
}

static void expect(const DevPool& pool, size_t blocks, int64_t resident, const char* what) {
  CHECK(live_blocks.size() == blocks && pool.live.size() == blocks, "%s: %zu blocks live in the allocator, %zu in the pool, expected %zu", what,
        live_blocks.size(), pool.live.size(), blocks);
  CHECK(pool.bytes_resident == resident, "%s: resident %lld, expected %lld", what, (long long)pool.bytes_resident, (long long)resident);
}

// ---- single buffers -------------------------------------------------------------------------------------------------------
static void check_single() {
  DevPool pool;
  pool.owner = &owner_told;
  pool.refused = refused;
  DevBuf<double> b;
  CHECK(b.reserve(pool, 10) == 0 && b.cap == 10 && b.p, "first reserve");
  b[9] = 1.0;  // (the conversion to T*; one past would be an AddressSanitizer report)
  expect(pool, 1, 80, "reserve 10");
  double* first = b;
  const int a0 = allocs_seen;
  CHECK(b.reserve(pool, 10) == 0 && b.reserve(pool, 3) == 0 && b.p == first && b.cap == 10 && allocs_seen == a0, "reserve of what is there is a no-op");
  CHECK(b.reserve(pool, 11) == 0 && b.cap == 11, "grow");
  expect(pool, 1, 88, "grow to exactly 11");
  // stale: the block stays, and stays counted, until the next reserve exchanges it
  b.stale();
  CHECK(b.cap == 0 && b.p, "stale keeps the pointer");
  expect(pool, 1, 88, "stale");
  const int f0 = frees_seen;
  CHECK(b.reserve(pool, 4) == 0 && b.cap == 4 && frees_seen == f0 + 1, "reserve after stale replaces the block");
  expect(pool, 1, 32, "reserve 4 after stale");
  // renew: always a fresh block; need < 1 gives one element
  const int a1 = allocs_seen;
  CHECK(b.renew(pool, 4) == 0 && allocs_seen == a1 + 1 && b.cap == 4, "renew of the same size allocates");
  CHECK(b.renew(pool, 0) == 0 && b.cap == 1, "renew(0) holds one element");
  expect(pool, 1, 8, "renew 0");
  CHECK(pool.bytes_peak == 88, "peak %lld", (long long)pool.bytes_peak);
  // a failing allocation: the old block is gone (freed first), the buffer is empty, the owner was told
  const int told = owner_told;
  fail_in = 1;
  CHECK(b.reserve(pool, 100) == -7 && !b.p && b.cap == 0 && owner_told == told + 1, "failed reserve leaves the buffer empty");
  expect(pool, 0, 0, "failed reserve");
  CHECK(b.reserve(pool, 100) == 0 && b.cap == 100, "retry");
  b.drop(pool);
  CHECK(!b.p && b.cap == 0, "drop");
  b.drop(pool);  // of an empty buffer: nothing
  expect(pool, 0, 0, "drop");
  std::printf("single buffer: reserve / stale / renew / failure / drop agree\n");
}

// ---- adopt, and a temporary abandoned by an early return ------------------------------------------------------------------
static int grow_into(DevPool& pool, DevBuf<int32_t>& owner, int64_t n, bool give_up) {
  ScopedBuf<int32_t> tmp(pool);
  const int rc = tmp.reserve(pool, n);
  if (rc) return rc;
  for (int64_t i = 0; i < n; ++i) tmp[i] = (int32_t)i;
  if (give_up) return 1;  // the early return: tmp's block goes back here
  owner.adopt(pool, tmp);
  return 0;
}

static void check_adopt() {
  DevPool pool;
  pool.owner = &owner_told;
  pool.refused = refused;
  DevBuf<int32_t> b;
  CHECK(b.reserve(pool, 5) == 0, "reserve");
  CHECK(grow_into(pool, b, 9, true) == 1 && b.cap == 5, "abandoned");
  expect(pool, 1, 20, "abandoned temporary");
  CHECK(grow_into(pool, b, 9, false) == 0 && b.cap == 9 && b[8] == 8, "adopted");
  expect(pool, 1, 36, "adopted temporary");
  CHECK(pool.bytes_peak == 56, "both copies coexisted: peak %lld", (long long)pool.bytes_peak);
  fail_in = 1;
  CHECK(grow_into(pool, b, 20, false) == -7 && b.cap == 9, "a temporary that could not be had leaves the owner alone");
  expect(pool, 1, 36, "failed temporary");
  DevBuf<int32_t> empty;
  CHECK(grow_into(pool, empty, 2, false) == 0 && empty.cap == 2, "adopt into an empty buffer");
  pool.release_all();
  expect(pool, 0, 0, "release_all");
  std::printf("adopt / abandon agree\n");
}

// ---- a row group ----------------------------------------------------------------------------------------------------------
struct Group : RowGroup {
  DevBuf<double> a, b;
  DevBuf<int32_t> c;
  DevBuf<double> d;
  int reserve(DevPool& pool, int64_t n) {
    return reserve_rows(n, [&] {
      int rc;
      if ((rc = a.renew(pool, 3 * n)) || (rc = b.renew(pool, n)) || (rc = c.renew(pool, 2 * n))) return rc;
      return d.renew(pool, n);
    });
  }
};

static void check_group() {
  const int64_t bytes_at = 8 * 3 + 8 + 4 * 2 + 8, members = 4;  // bytes per row of the group
  for (int k = 1; k <= members; ++k) {
    DevPool pool;
    pool.owner = &owner_told;
  pool.refused = refused;
    Group g;
    CHECK(g.reserve(pool, 6) == 0 && g.rows == 6, "group reserve");
    expect(pool, members, 6 * bytes_at, "group of 6 rows");
    const int a0 = allocs_seen;
    CHECK(g.reserve(pool, 6) == 0 && g.reserve(pool, 2) == 0 && allocs_seen == a0, "a group that is large enough is left alone");
    fail_in = k;  // growing: member k cannot be had
    CHECK(g.reserve(pool, 10) == -7 && g.rows == 0, "member %d failed: no rows claimed (rows = %lld)", k, (long long)g.rows);
    CHECK(live_blocks.size() == pool.live.size() && (int)pool.live.size() == members - 1, "member %d failed: %zu blocks, all known to the pool", k,
          pool.live.size());
    CHECK(g.reserve(pool, 10) == 0 && g.rows == 10, "retry after member %d failed", k);
    g.a[3 * 10 - 1] = 1.0, g.b[9] = 1.0, g.c[19] = 1, g.d[9] = 1.0;
    expect(pool, members, 10 * bytes_at, "group of 10 rows");
    g.stale();
    expect(pool, members, 10 * bytes_at, "a stale group still holds its blocks");
    CHECK(g.reserve(pool, 1) == 0 && g.rows == 1, "reserve after stale");
    expect(pool, members, 1 * bytes_at, "group of 1 row");
    pool.release_all();
    expect(pool, 0, 0, "release_all");
  }
  std::printf("row group: a failure at each of %lld members claims nothing and leaks nothing\n", (long long)members);
}

// ---- the ledger ------------------------------------------------------------------------------------------------------------
static void check_ledger() {
  DevPool pool;
  pool.owner = &owner_told;
  pool.refused = refused;
  DevBuf<double> scal, plan, x, y;
  CHECK(scal.renew(pool, 100, false) == 0 && plan.renew(pool, 7, false) == 0, "uncounted blocks");
  expect(pool, 2, 0, "uncounted blocks are not resident bytes");
  CHECK(pool.bytes_peak == 0, "... nor peak bytes");
  CHECK(x.reserve(pool, 10) == 0 && y.reserve(pool, 20) == 0, "counted blocks");
  expect(pool, 4, 240, "counted beside uncounted");
  plan.drop(pool);
  CHECK(plan.renew(pool, 9, false) == 0, "a plan rebuilt");
  expect(pool, 4, 240, "an uncounted block replaced");
  y.drop(pool);
  expect(pool, 3, 80, "drop of a counted block");
  CHECK(pool.bytes_peak == 240, "peak %lld", (long long)pool.bytes_peak);
  pool.release_all();  // what gmb_destroy does: counted, uncounted, whoever holds them
  expect(pool, 0, 0, "release_all");
  CHECK(pool.bytes_peak == 240, "the peak outlives the blocks");
  std::printf("ledger: counted / uncounted / peak agree\n");
}

int main() {
  check_single();
  check_adopt();
  check_group();
  check_ledger();
  CHECK(live_blocks.empty(), "%zu blocks live at exit", live_blocks.size());
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("buffer ownership agrees (%d allocations, %d frees)\n", allocs_seen, frees_seen);
  return 0;
}
