// laplace_plan_check.cpp -- the index arithmetic of the Laplace path (gumbi_amd/csrc/laplace_plan.hpp: the tiles of the lower
// triangle, the workspace slot of each, the parts a block row's sum adds and their order -- the very functions the kernels of
// laplace.hpp and engine.hip call) as a stand-alone program for the sanitizers.  No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/laplace_plan_check.cpp -o /tmp/laplace_plan_check
//   /tmp/laplace_plan_check
//
// Driven over a grid of N, sizes that must be refused included.  For every accepted plan: the padded sizes; every tile (I, J),
// J <= I, has a slot of its own inside the workspace (a vector of marks is really allocated and indexed as symv_lower_kernel
// indexes its slots); the nt + 1 parts of every block row lie inside the workspace, are the row parts of that row's tiles in
// ascending J followed by the column parts of that column's tiles in ascending I, and over all block rows every half of every slot
// is added exactly once; then a
// symmetric product carried out on the host through the plan (small integers, exact in double) against the dense one, the
// padding rows included; the likelihood pass's partial sets; the dump's capacity.  One line per failure; exit status 0 when all
// agree (tests/test_laplace_cpu.py builds and runs it plain and under the sanitizers).
#include <cstdio>
#include <vector>

#include "../gumbi_amd/csrc/laplace_plan.hpp"

using namespace gmb;

static int failures = 0;

static void bad(const char* what, long long n) {
  std::printf("FAIL %s (N = %lld)\n", what, n);
  ++failures;
}

// out = A v through the plan, as the two kernels do it: tile (I, J) leaves its row part and its column part in its slot (a
// diagonal tile: elements i >= j and i > j), block row R adds its parts in the plan's order
static void symv_by_plan(const LaplacePlan& pl, const std::vector<double>& A, const std::vector<double>& v, std::vector<double>& out) {
  const int64_t n = pl.N, T = LAP_TILE;
  std::vector<double> ws((size_t)pl.symv_doubles(), -1e300);  // (a part that is read before it is written shows)
  for (int64_t I = 0; I < pl.nt; ++I)
    for (int64_t J = 0; J <= I; ++J) {
      double* slot = ws.data() + lap_slot(I, J) * LAP_SLOT;
      for (int64_t k = 0; k < LAP_SLOT; ++k) slot[k] = 0.0;
      for (int64_t il = 0; il < T; ++il)
        for (int64_t jl = 0; jl < T; ++jl) {
          const int64_t gi = I * T + il, gj = J * T + jl;
          if (gi >= n || gj >= n || (I == J && jl > il)) continue;
          const double x = A[(size_t)(gi * n + gj)];
          slot[il] += x * v[(size_t)gj];
          if (!(I == J && jl == il)) slot[T + jl] += x * v[(size_t)gi];
        }
    }
  out.assign((size_t)pl.Np, 0.0);
  for (int64_t R = 0; R < pl.nt; ++R)
    for (int64_t t = 0; t < T; ++t) {
      double s = 0.0;
      for (int64_t q = 0; q < lap_terms(pl.nt); ++q) s += ws[(size_t)(lap_term_offset(R, q) + t)];
      out[(size_t)(R * T + t)] = R * T + t < n ? s : 0.0;
    }
}

static void check(int64_t N, int want, bool product) {
  LaplacePlan pl;
  const int rc = pl.make(N);
  if (rc != want) return bad("status of make", N);
  if (rc) return;
  if (pl.Np % LAP_TILE || pl.Np < N || pl.Np - N >= LAP_TILE) return bad("Np", N);
  if (pl.Nr % LAP_TILE || pl.Nr < N + 1 || pl.Nr - (N + 1) >= LAP_TILE) return bad("Nr", N);
  if (pl.nt * LAP_TILE != pl.Np || pl.slots != pl.nt * (pl.nt + 1) / 2) return bad("tiles", N);
  if (pl.lik_blocks * LAP_LIK_BLOCK < pl.Np || (pl.lik_blocks - 1) * LAP_LIK_BLOCK >= pl.Np) return bad("likelihood blocks", N);
  if (pl.nt <= 512) {
    // every tile a slot of its own
    std::vector<unsigned char> marks((size_t)pl.slots, 0);
    for (int64_t I = 0; I < pl.nt; ++I)
      for (int64_t J = 0; J <= I; ++J) {
        const int64_t s = lap_slot(I, J);
        if (s < 0 || s >= pl.slots) return bad("slot out of range", N);
        ++marks[(size_t)s];
      }
    for (unsigned char c : marks)
      if (c != 1) return bad("a slot used other than once", N);
    // every half of every slot is a part of exactly one block row
    std::vector<unsigned char> halves((size_t)(2 * pl.slots), 0);
    for (int64_t R = 0; R < pl.nt; ++R)
      for (int64_t q = 0; q < lap_terms(pl.nt); ++q) {
        const int64_t off = lap_term_offset(R, q);
        if (off < 0 || off % LAP_TILE || off + LAP_TILE > (int64_t)pl.symv_doubles()) return bad("part out of range", N);
        const int64_t want_off = q <= R ? lap_slot(R, q) * LAP_SLOT : lap_slot(q - 1, R) * LAP_SLOT + LAP_TILE;
        if (off != want_off) return bad("order of a block row's parts", N);
        ++halves[(size_t)(off / LAP_TILE)];
      }
    for (unsigned char c : halves)
      if (c != 1) return bad("a part added other than once", N);
  }
  if (product) {
    std::vector<double> A((size_t)(N * N)), v((size_t)N), out, dense((size_t)N, 0.0);
    for (int64_t i = 0; i < N; ++i) {
      v[(size_t)i] = (double)((i * 7 + 3) % 11 - 5);
      for (int64_t j = 0; j <= i; ++j) A[(size_t)(i * N + j)] = A[(size_t)(j * N + i)] = (double)((i * 31 + j * 17 + i * j) % 13 - 6);
    }
    for (int64_t i = 0; i < N; ++i)
      for (int64_t j = 0; j < N; ++j) dense[(size_t)i] += A[(size_t)(i * N + j)] * v[(size_t)j];
    symv_by_plan(pl, A, v, out);
    for (int64_t i = 0; i < pl.Np; ++i)
      if (out[(size_t)i] != (i < N ? dense[(size_t)i] : 0.0)) return bad("the product through the plan", N);
  }
  const int64_t need = laplace_plan_dump(pl, 0.0, nullptr, 0);
  if (need != LAP_DUMP_HEADER + pl.nt * (pl.nt + 1)) return bad("length of the dump", N);
  if (need <= 4096) {
    std::vector<int64_t> buf((size_t)need + 1, -7);
    if (laplace_plan_dump(pl, 0.0, buf.data(), need - 1) != need || buf[(size_t)need - 1] != -7) return bad("the dump's capacity", N);
    if (laplace_plan_dump(pl, 0.0, buf.data(), need) != need || buf[(size_t)need] != -7 || buf[0] != pl.Np || buf[3] != pl.slots)
      return bad("the dump", N);
  }
}

int main() {
  check(0, 1, false);
  check(-5, 1, false);
  check(LAP_MAX_N + 1, 2, false);
  for (int64_t N : {1, 2, 100, 127, 128, 129, 255, 256, 257, 300, 383, 384, 385, 640}) check(N, 0, true);
  for (int64_t N : {(int64_t)10000, (int64_t)50000, (int64_t)65536, LAP_MAX_N}) check(N, 0, false);
  if (failures) return 1;
  std::printf("laplace_plan_check: all plans agree\n");
  return 0;
}
