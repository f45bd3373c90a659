// fitc_plan_check.cpp -- the index arithmetic of the sparse (FITC) path (gumbi_amd/csrc/fitc_plan.hpp: the column tiles of X, the
// padded sizes, the partial-sum blocks -- the very functions engine.hip calls before anything is launched) as a stand-alone
// program for the sanitizers.  No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/fitc_plan_check.cpp -o /tmp/fitc_plan_check
//   /tmp/fitc_plan_check
//
// Driven over a grid of (N, m), sizes that must be refused included.  For every accepted plan: the tiles cover the columns
// 0 .. N - 1 once and in order, each starts on a multiple of 128, is padded by less than a tile, fits the workspace rows the plan
// asks for and -- with its padding -- ends inside the per-column vectors; an m x tile block stays within the byte bound unless the
// tile is the smallest there is; the blocks of 32 columns of the column kernels are written once each (a vector of marks is
// really allocated and indexed as the kernels index their partial sums); the derivative reduction's workgroups fit the count the
// plan reserves; the dump respects its capacity.  One line per failure; exit status 0 when all agree (tests/test_fitc_cpu.py builds
// and runs it plain and under the sanitizers).
#include <cstdio>
#include <vector>

#include "../gumbi_amd/csrc/fitc_plan.hpp"

using namespace gmb;

static int failures = 0;

static void bad(const char* what, long long n, long long m) {
  std::printf("FAIL %s (N = %lld, m = %lld)\n", what, n, m);
  ++failures;
}

static void check(int64_t N, int64_t m, int want) {
  FitcPlan pl;
  const int rc = pl.make(N, m);
  if (rc != want) return bad("status of make", N, m);
  if (rc) return;
  if (pl.Np % FITC_TILE || pl.Np < N || pl.Np - N >= FITC_TILE) return bad("Np", N, m);
  if (pl.mp % FITC_TILE || pl.mp < m || pl.mp - m >= FITC_TILE) return bad("mp", N, m);
  if (pl.mr % FITC_TILE || pl.mr < m + 1 || pl.mr - (m + 1) >= FITC_TILE) return bad("mr", N, m);
  if (pl.tile_rows % FITC_TILE || pl.tile_rows < FITC_TILE || pl.tile_rows > FITC_MAX_TILE_ROWS) return bad("tile rows", N, m);
  if (pl.tile_rows > FITC_TILE && 8.0 * (double)pl.tile_rows * (double)pl.mr > FITC_BLOCK_BYTES) return bad("block bytes", N, m);
  if (pl.tmax > pl.tile_rows || pl.tmax > pl.Np || pl.tmax % FITC_TILE) return bad("workspace rows", N, m);
  std::vector<unsigned char> marks((size_t)pl.col_blocks(), 0);
  int64_t next = 0;
  for (int64_t t = 0; t < pl.ntile; ++t) {
    const FitcTile tl = pl.tile(t);
    if (tl.first != next || tl.count < 1) return bad("tile order", N, m);
    if (tl.first % FITC_TILE || tl.tpad % FITC_TILE || tl.tpad < tl.count || tl.tpad - tl.count >= FITC_TILE) return bad("tile padding", N, m);
    if (tl.tpad > pl.tmax || tl.first + tl.tpad > pl.Np) return bad("tile extent", N, m);
    if (t + 1 < pl.ntile && tl.count != pl.tile_rows) return bad("a ragged tile that is not the last", N, m);
    // the column kernels: tpad / 32 workgroups, workgroup b writes the partial sums of block first / 32 + b
    for (int64_t b = 0; b < tl.tpad / FITC_COL_BLOCK; ++b) ++marks[(size_t)(tl.first / FITC_COL_BLOCK + b)];
    // the derivative reduction of this tile against Z
    if ((tl.tpad / FITC_TILE) * (pl.mp / FITC_TILE) > pl.deriv_blocks()) return bad("derivative workgroups of a tile", N, m);
    next += tl.count;
  }
  if (next != N) return bad("coverage", N, m);
  for (unsigned char c : marks)
    if (c != 1) return bad("a block of columns written other than once", N, m);
  if ((pl.mp / FITC_TILE) * (pl.mp / FITC_TILE) > pl.deriv_blocks()) return bad("derivative workgroups of Z x Z", N, m);
  for (int64_t M : {(int64_t)1, (int64_t)129, pl.tile_rows, pl.tile_rows + 1, (int64_t)1 << 33}) {
    const int64_t mt = pl.predict_rows(M);
    if (mt % FITC_TILE || mt < FITC_TILE || mt > pl.tile_rows || (M <= pl.tile_rows && mt < M)) return bad("prediction tile", N, m);
  }
  // the dump: its length, and nothing written beyond the capacity
  const int64_t len = FITC_DUMP_HEADER + 3 * pl.ntile;
  if (fitc_plan_dump(pl, 1.0, 2.0, 3.0, nullptr, 0) != len) return bad("dump size", N, m);
  std::vector<int64_t> out((size_t)len + 2, -7);
  if (fitc_plan_dump(pl, 1.0, 2.0, 3.0, out.data(), len - 1) != len || out[(size_t)len - 1] != -7 || out[(size_t)len] != -7)
    return bad("dump capacity", N, m);
  fitc_plan_dump(pl, 1.0, 2.0, 3.0, out.data(), len);
  const FitcTile last = pl.tile(pl.ntile - 1);
  if (out[0] != pl.Np || out[3] != pl.tile_rows || out[5] != pl.ntile || out[7] != 1 || out[9] != 3 || out[(size_t)len - 3] != last.first ||
      out[(size_t)len - 2] != last.count || out[(size_t)len - 1] != last.tpad)
    return bad("dump contents", N, m);
}

int main() {
  const int64_t Ns[] = {1, 2, 127, 128, 129, 700, 4096, 32767, 32768, 32769, 65536, 65537, 100000, 1000000, 3000001};
  const int64_t ms[] = {1, 2, 16, 127, 128, 129, 130, 512, 1024, 4095, 8064, 8065, 16383, 16384};
  for (int64_t N : Ns)
    for (int64_t m : ms) check(N, m, 0);
  check(0, 5, 1);
  check(-3, 5, 1);
  check(10, 0, 2);
  check(10, -1, 2);
  check(10, FITC_MAX_M + 1, 3);
  check(((int64_t)1 << 40) + 1, 5, 4);
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("fitc_plan_check: all plans agree\n");
  return 0;
}
