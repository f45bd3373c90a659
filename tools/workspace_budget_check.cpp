// workspace_budget_check.cpp -- the engine's workspaces and the budgets of its guarded calls (gumbi_amd/csrc/workspaces.hpp and the
// Budget / Reserver of device_buffers.hpp: the very headers engine.hip sizes, measures and allocates with) driven over a HOST
// allocator, as a stand-alone program for the sanitizers.  No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/workspace_budget_check.cpp -o /tmp/workspace_budget_check
//   /tmp/workspace_budget_check
//
// The allocator hooks are malloc / free with a live set of their own (as in tools/device_buffers_check.cpp), and the allocator can
// be told to fail its k-th allocation from now.  Checked:
//   (a) every workspace struct, over a grid of sizes: bytes() is what reserve() adds to the pool's ledger; the budget's "still to
//       allocate", taken BEFORE a growth, is what the growth adds; a stale workspace counts in full;
//   (b) the budgets of the guarded calls -- joint posterior, leave-out, group averages with and without covariance, product form,
//       host staging -- against the byte formulas those guards were written with before they walked a list.  The formulas live
//       HERE now, and only here: the independent reference;
//   (c) a member allocation that fails half-way leaves no rows claimed and nothing leaked, and the retry succeeds -- on the real
//       structs and through a whole call's list.
// One line per case; exit status 0 when all agree (tests/test_workspace_budget_cpu.py builds and runs it without the sanitizers).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>

#define GMB_DEVBUF_OWN_HOOKS  // the allocator is this file's
#include "../gumbi_amd/csrc/workspaces.hpp"

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
static int fail_in = 0;  // > 0: the fail_in-th allocation from now fails

const char* gmb::devbuf_alloc(void** p, size_t bytes) {
  if (fail_in > 0 && --fail_in == 0) return "told to fail";
  *p = std::malloc(bytes);
  CHECK(*p != nullptr && bytes > 0, "malloc of %zu bytes", bytes);
  live_blocks.insert(*p);
  return nullptr;
}
void gmb::devbuf_free(void* p) {
  if (!live_blocks.count(p)) {
    CHECK(false, "double free or free of unknown block %p", p);
    return;
  }
  live_blocks.erase(p);
  std::free(p);
}
static int refused(void*, size_t, const char*) { return -7; }
static void own(DevPool& pool) { pool.refused = refused; }

// ---- (a) + (c): one workspace struct --------------------------------------------------------------------------------------------
static const int64_t ROWS[] = {128, 256, 4096};

template <class W, class... A>
static int count_members(W& w, A... a) {
  int n = 0;
  w.each(1.0, a..., [&](auto&, double) { return ++n, true; });
  return n;
}

template <class W, class... A>
static void check_struct(const char* name, A... a) {
  for (int64_t r1 : ROWS)
    for (int64_t r2 : ROWS) {
      if (r2 <= r1) continue;
      DevPool pool;
      own(pool);
      W w;
      const int members = count_members(w, a...);
      CHECK(w.reserve(pool, r1, a...) == 0 && w.rows == r1, "%s: reserve %lld", name, (long long)r1);
      CHECK((double)pool.bytes_resident == w.bytes((double)r1, a...) && (int)pool.live.size() == members, "%s: bytes(%lld) = %.0f, ledger %lld",
            name, (long long)r1, w.bytes((double)r1, a...), (long long)pool.bytes_resident);
      Budget grow;
      grow.rows(w, (double)r2, a...);
      Budget fits;  // a request it serves already: nothing to allocate
      fits.rows(w, (double)r1, a...);
      CHECK(fits.fresh == 0.0 && fits.total == w.bytes((double)r1, a...), "%s: a workspace that is large enough needs nothing", name);
      const int64_t before = pool.bytes_resident;
      // (c) growing, member k cannot be had: no rows, nothing leaked -- and then the growth itself
      for (int k = 1; k <= members; ++k) {
        W v;
        DevPool p2;
        own(p2);
        const size_t held = live_blocks.size();
        CHECK(v.reserve(p2, r1, a...) == 0, "%s: reserve", name);
        fail_in = k;
        CHECK(v.reserve(p2, r2, a...) == -7 && v.rows == 0, "%s: member %d failed: no rows claimed", name, k);
        CHECK(live_blocks.size() - held == p2.live.size() && (int)p2.live.size() == members - 1, "%s: member %d failed: %zu blocks", name, k, p2.live.size());
        Budget all;
        all.rows(v, (double)r2, a...);
        CHECK(all.fresh == v.bytes((double)r2, a...), "%s: after a failure the budget counts the workspace in full", name);
        CHECK(v.reserve(p2, r2, a...) == 0 && v.rows == r2 && (double)p2.bytes_resident == v.bytes((double)r2, a...), "%s: retry after member %d", name, k);
        p2.release_all();
      }
      CHECK(w.reserve(pool, r2, a...) == 0 && w.rows == r2, "%s: grow to %lld", name, (long long)r2);
      CHECK(grow.fresh == (double)(pool.bytes_resident - before) && grow.total == (double)pool.bytes_resident,
            "%s: %lld -> %lld rows: budget %.0f fresh of %.0f, ledger grew %lld to %lld", name, (long long)r1, (long long)r2, grow.fresh, grow.total,
            (long long)(pool.bytes_resident - before), (long long)pool.bytes_resident);
      w.stale();
      Budget stale;
      stale.rows(w, (double)r2, a...);
      CHECK(stale.fresh == w.bytes((double)r2, a...) && stale.total == stale.fresh, "%s: a stale workspace counts in full (%.0f)", name, stale.fresh);
      CHECK(w.reserve(pool, r2, a...) == 0 && (double)pool.bytes_resident == stale.total && (int)pool.live.size() == members, "%s: reserve after stale", name);
      pool.release_all();
    }
  CHECK(live_blocks.empty(), "%s: %zu blocks left", name, live_blocks.size());
}

static void check_structs() {
  check_struct<PreparedPoints>("PreparedPoints");
  for (int64_t Np : {(int64_t)128, (int64_t)4224})
    for (int D : {1, 5}) {
      check_struct<PredictWorkspace>("PredictWorkspace", Np, D);
      check_struct<GemmFormWorkspace>("GemmFormWorkspace", Np);
      check_struct<PredictGradWorkspace>("PredictGradWorkspace", D);
      check_struct<GroupWorkspace>("GroupWorkspace", D);
      for (int nt : {1, 5}) check_struct<TermsWorkspace>("TermsWorkspace", (int64_t)red_chunks(Np) * tg_entries(nt));
      for (bool cov : {false, true}) check_struct<SlopeWorkspace>("SlopeWorkspace", (int64_t)red_chunks(Np) * (cov ? 20 : 10), D, cov);
    }
  // a workspace whose SHAPE grows holds nothing for the new shape, whatever its rows: counted in full, renewed in full
  DevPool pool;
  own(pool);
  TermsWorkspace tg;
  const int64_t one = 17 * tg_entries(1), five = 17 * tg_entries(5);  // 17 chunks, 1 and 5 terms
  CHECK(tg.reserve(pool, 256, one) == 0 && tg.held(one) == 256 && tg.held(five) == 0 && tg.held(one - 1) == 256, "terms: held by shape");
  Budget b;
  b.rows(tg, 128.0, five);
  CHECK(b.fresh == tg.bytes(128.0, five), "terms: more entries per row count in full");
  CHECK(tg.reserve(pool, 128, five) == 0 && tg.rows == 128 && (double)pool.bytes_resident == b.total, "terms: renewed for the new shape");
  SlopeWorkspace sl;
  CHECK(sl.reserve(pool, 256, 40, 3, false) == 0 && sl.held(40, 3, false) == 256 && sl.held(40, 3, true) == 0 && sl.held(41, 3, false) == 0, "slope: held by shape");
  const int64_t before = pool.bytes_resident;
  CHECK(sl.reserve(pool, 128, 40, 3, true) == 0 && sl.rows == 128 && sl.has_cov && (double)(pool.bytes_resident - before) == sl.bytes(128.0, 40, 3, true) - sl.bytes(256.0, 40, 3, false),
        "slope: renewed with its covariance");
  pool.release_all();
  std::printf("workspaces: bytes() = ledger, budget before a growth = the growth, stale counts in full, a failed member claims nothing\n");
}

// ---- (b): the guarded calls ---------------------------------------------------------------------------------------------------------
struct MockEngine {  // what the lists use of the engine
  int64_t N = 0, Np = 0;
  int32_t D = 0;
  DevPool pool;
  PredictWorkspace pw;
  GemmFormWorkspace pw2;
  DevBuf<double> dpart;
  struct {
    DevBuf<double> dC, dstage;
  } jt;
  GroupWorkspace ga;
  DevBuf<double> ga_part;
  DevBuf<int64_t> ga_idx;
};

static int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
constexpr int64_t TILE = 128;

struct Bytes {
  double total, fresh;
};

// the guards' arithmetic as it was written out by hand, one function per guard
static Bytes formula_joint(const MockEngine& e, int64_t M, bool gemm_form, double stage) {
  const double Mr = (double)round_up(M + 1, TILE), Mp = (double)round_up(M, TILE), Np = (double)e.Np;
  const int nchunk = (int)((e.N + RED_CHUNK - 1) / RED_CHUNK);
  const double per_row = 8.0 * (Np + e.D + 17 + MAX_LIN + 3) + 4.0 * MAX_TABS;
  const double v_bytes = 8.0 * Mr * Np, c_bytes = 8.0 * Mr * Mp, stage_bytes = 8.0 * stage;
  const double total = per_row * Mr + 16.0 * nchunk * Mr + (gemm_form ? v_bytes : 0.0) + c_bytes + stage_bytes;
  double fresh = 0.0;
  if ((double)e.pw.rows < Mr) fresh += per_row * (Mr - (double)e.pw.rows);
  if ((double)e.dpart.cap < 2.0 * nchunk * Mr) fresh += 8.0 * (2.0 * nchunk * Mr - (double)e.dpart.cap);
  if (gemm_form && (double)e.pw2.rows < Mr) fresh += 8.0 * Np * (Mr - (double)e.pw2.rows);
  if ((double)e.jt.dC.cap < Mr * Mp) fresh += 8.0 * (Mr * Mp - (double)e.jt.dC.cap);
  if ((double)e.jt.dstage.cap < stage) fresh += 8.0 * (stage - (double)e.jt.dstage.cap);
  return {total, fresh};
}

static Bytes formula_leave_out(const MockEngine& e, int64_t Mt) {
  const int nchunk = (int)((e.N + RED_CHUNK - 1) / RED_CHUNK);
  const double per_row = 8.0 * ((double)e.Np + e.D + 17 + MAX_LIN + 3) + 4.0 * MAX_TABS;
  double fresh = 0.0;
  if (e.pw.rows < Mt) fresh += per_row * (double)(Mt - e.pw.rows);
  if ((double)e.dpart.cap < 2.0 * nchunk * (double)Mt) fresh += 8.0 * (2.0 * nchunk * (double)Mt - (double)e.dpart.cap);
  return {per_row * (double)Mt + 16.0 * nchunk * (double)Mt, fresh};
}

static Bytes formula_group(const MockEngine& e, int64_t M, int64_t G, int64_t ntask, int64_t block_tasks, bool gemm_form, bool with_cov, double stage) {
  const int64_t mp = round_up(M, TILE), gr = round_up(G + 1, TILE), gp = round_up(G, TILE);
  const double Mp = (double)mp, Gr = (double)gr, Gp = (double)gp, Np = (double)e.Np;
  const int nchunk = (int)((e.N + RED_CHUNK - 1) / RED_CHUNK);
  const double ga_row = 8.0 * (e.D + 17 + MAX_LIN + 1 + GA_ROWS) + 4.0 * MAX_TABS;
  const double part = std::max((double)ntask * Np, (double)block_tasks * Mp);
  const double idx = 3.0 * (double)ntask + 2.0 * (double)(G + 1);
  const double per_row = 8.0 * (Np + e.D + 17 + MAX_LIN + 3) + 4.0 * MAX_TABS;
  const double total = ga_row * Mp + 8.0 * part + 8.0 * idx + per_row * Gr + 16.0 * nchunk * Gr + (gemm_form ? 8.0 * Gr * Np : 0.0) +
                       (with_cov ? 8.0 * Gr * Gp + 8.0 * stage : 0.0);
  double fresh = 0.0;
  if ((double)e.ga.rows < Mp) fresh += ga_row * (Mp - (double)e.ga.rows);
  if ((double)e.ga_part.cap < part) fresh += 8.0 * (part - (double)e.ga_part.cap);
  if ((double)e.ga_idx.cap < idx) fresh += 8.0 * (idx - (double)e.ga_idx.cap);
  if ((double)e.pw.rows < Gr) fresh += per_row * (Gr - (double)e.pw.rows);
  if ((double)e.dpart.cap < 2.0 * nchunk * Gr) fresh += 8.0 * (2.0 * nchunk * Gr - (double)e.dpart.cap);
  if (gemm_form && (double)e.pw2.rows < Gr) fresh += 8.0 * Np * (Gr - (double)e.pw2.rows);
  if (with_cov && (double)e.jt.dC.cap < Gr * Gp) fresh += 8.0 * (Gr * Gp - (double)e.jt.dC.cap);
  if (with_cov && (double)e.jt.dstage.cap < stage) fresh += 8.0 * (stage - (double)e.jt.dstage.cap);
  return {total, fresh};
}

// the lists, called as engine.hip calls them
template <class V>
static bool list_joint(MockEngine& e, int64_t M, bool gemm_form, double stage, V& v) {
  return joint_buffers(e, (double)round_up(M + 1, TILE), (double)round_up(M, TILE), gemm_form, stage, v);
}
template <class V>
static bool list_group(MockEngine& e, int64_t M, int64_t G, int64_t ntask, int64_t block_tasks, bool gemm_form, bool with_cov, double stage, V& v) {
  return group_buffers(e, (double)round_up(M, TILE), (double)G, (double)round_up(G + 1, TILE), (double)round_up(G, TILE), (double)ntask,
                       (double)block_tasks, gemm_form, with_cov, stage, v);
}

// every request against the engine as it stands: budget == formula, exactly (all of these are integers below 2^53)
static int compare_all(MockEngine& e, const char* state) {
  int cases = 0;
  auto same = [&](const char* what, const Budget& b, const Bytes& f, long long M, long long G) {
    ++cases;
    CHECK(b.total == f.total && b.fresh == f.fresh, "%s, %s M = %lld G = %lld: budget %.0f / %.0f, formula %.0f / %.0f", state, what, M, G, b.total,
          b.fresh, f.total, f.fresh);
  };
  for (int64_t M : {(int64_t)1, (int64_t)127, (int64_t)128, (int64_t)700, (int64_t)5000})
    for (bool gemm_form : {false, true}) {
      for (double stage : {0.0, (double)M * (double)M, 2.0 * 33.0 * (double)M}) {
        Budget b;
        list_joint(e, M, gemm_form, stage, b);
        same("joint", b, formula_joint(e, M, gemm_form, stage), M, 0);
      }
      for (int64_t G : {(int64_t)1, (int64_t)127, (int64_t)300, M})
        for (bool with_cov : {false, true})
          for (bool host : {false, true}) {
            if (G > M) continue;
            const int64_t ntask = G + (M - G) / 512 + 1, block_tasks = std::min<int64_t>(ntask, 160);
            const double stage = host && with_cov ? (double)G * (double)G : 0.0;
            Budget b;
            list_group(e, M, G, ntask, block_tasks, gemm_form, with_cov, stage, b);
            same("groups", b, formula_group(e, M, G, ntask, block_tasks, gemm_form, with_cov, stage), M, G);
          }
    }
  for (int64_t Mt : {(int64_t)128, (int64_t)1024, (int64_t)8192}) {
    Budget b;
    predict_buffers(e, (double)Mt, b);
    same("leave-out", b, formula_leave_out(e, Mt), Mt, 0);
  }
  return cases;
}

static void check_calls() {
  int cases = 0;
  for (int64_t N : {(int64_t)300, (int64_t)4224})
    for (int D : {1, 5}) {
      MockEngine e;
      own(e.pool);
      e.N = N, e.Np = round_up(N, TILE), e.D = D;
      cases += compare_all(e, "empty");
      // partly grown: a joint posterior at 200 points in the product form with staging, then group averages without covariance.
      // What the budget said before each is what the ledger gained.
      Reserver take{e.pool};
      Budget b1;
      list_joint(e, 200, true, 200.0 * 200.0, b1);
      CHECK(list_joint(e, 200, true, 200.0 * 200.0, take) && take.rc == 0 && (double)e.pool.bytes_resident == b1.fresh && b1.fresh == b1.total, "joint on an empty engine");
      cases += compare_all(e, "after a joint posterior");
      Budget b2;
      list_group(e, 900, 300, 303, 130, false, false, 0.0, b2);
      const int64_t before = e.pool.bytes_resident;
      CHECK(list_group(e, 900, 300, 303, 130, false, false, 0.0, take) && take.rc == 0 && (double)(e.pool.bytes_resident - before) == b2.fresh, "groups after the joint posterior");
      cases += compare_all(e, "after group averages");
      // stale, as a change of N leaves the engine: the workspaces sized by N hold nothing, the second matrix stays
      e.pw.stale(), e.pw2.stale(), e.dpart.stale(), e.ga.stale();
      cases += compare_all(e, "stale");
      // (c) through a whole call's list: the k-th allocation fails, nothing leaks, the retry leaves what the budget's total says
      for (int k = 1; k <= 12; ++k) {
        MockEngine f;
        own(f.pool);
        f.N = N, f.Np = e.Np, f.D = D;
        Reserver tk{f.pool};
        Budget all;
        list_group(f, 700, 40, 45, 45, true, true, 1600.0, all);
        const size_t held = live_blocks.size();
        fail_in = k;
        CHECK(!list_group(f, 700, 40, 45, 45, true, true, 1600.0, tk) && tk.rc == -7, "allocation %d of the groups call fails", k);
        CHECK(live_blocks.size() - held == f.pool.live.size(), "allocation %d failed: every block is known to the pool", k);
        CHECK(list_group(f, 700, 40, 45, 45, true, true, 1600.0, tk) && tk.rc == 0 && (double)f.pool.bytes_resident == all.total, "retry after allocation %d: %lld resident, %.0f budgeted", k,
              (long long)f.pool.bytes_resident, all.total);
        f.pool.release_all();
      }
      fail_in = 0;
      e.pool.release_all();
    }
  // a request beyond int64_t (Mr * Mp = 2^66): the budget stays finite and agrees with the formula to rounding (the sums run in
  // another order, and no longer over integers a double holds exactly)
  MockEngine e;
  e.N = 4224, e.Np = 4224, e.D = 2;
  const int64_t M = (int64_t)1 << 33;
  Budget b;
  list_joint(e, M, true, (double)M * (double)M, b);
  const Bytes f = formula_joint(e, M, true, (double)M * (double)M);
  CHECK(std::isfinite(b.total) && std::fabs(b.total - f.total) <= 1e-14 * f.total && std::fabs(b.fresh - f.fresh) <= 1e-14 * f.fresh,
        "M = 2^33: budget %.0f / %.0f, formula %.0f / %.0f", b.total, b.fresh, f.total, f.fresh);
  std::printf("guarded calls: %d budgets equal the hand-written formulas (empty, grown, stale); a failed allocation leaks nothing\n", cases);
}

int main() {
  check_structs();
  check_calls();
  CHECK(live_blocks.empty(), "%zu blocks live at exit", live_blocks.size());
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("workspace budgets agree\n");
  return 0;
}
