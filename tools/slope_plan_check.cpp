// slope_plan_check.cpp -- the index arithmetic of gmb_predict_slope (gumbi_amd/csrc/slope_plan.hpp: the differentiable columns, the
// M-tile and the stacked layout, the very functions engine.hip calls before anything is launched) as a stand-alone program for the
// sanitizers.  No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/slope_plan_check.cpp -o /tmp/slope_plan_check
//   /tmp/slope_plan_check
//
// Driven over a grid of (D, term layouts, M, Np): the column list is the sorted union of the terms' continuous and linear columns,
// each once, whatever order and however often they are added, and refuses a negative column and a 25th one; the M-tile is a
// multiple of 128, at least 128, and Dc tiles of it fit a prediction's largest tile whenever that holds Dc x 128 rows; every
// (column, point, training column) of every M-tile lands on its own element of a buffer of ldz x Np doubles -- the buffer is
// really allocated and every element written exactly once; the packed triangle and the 4 x 4 blocks of the (d, e) pairs cover
// every pair once.  One line per failure; exit status 0 when all agree (tests/test_predict_slope_cpu.py builds and runs it
// without the sanitizers).
#include <algorithm>
#include <cstdio>
#include <set>
#include <vector>

#include "../gumbi_amd/csrc/slope_plan.hpp"

using namespace gmb;

static int failures = 0;

static void bad(const char* what, long long a, long long b, long long c) {
  std::printf("FAIL %s (%lld, %lld, %lld)\n", what, a, b, c);
  ++failures;
}

// the union of a model's terms: `terms` lists of continuous columns and of linear columns
static void check_columns(int D, const std::vector<std::vector<int32_t>>& cont, const std::vector<std::vector<int32_t>>& lin) {
  SlopeColumns s;
  std::set<int32_t> want;
  for (size_t t = 0; t < cont.size(); ++t) {
    if (!slope_add_columns(s, cont[t].data(), (int)cont[t].size()) || !slope_add_columns(s, lin[t].data(), (int)lin[t].size()))
      return bad("columns refused", D, (long long)t, s.n);
    want.insert(cont[t].begin(), cont[t].end());
    want.insert(lin[t].begin(), lin[t].end());
  }
  if (s.n != (int)want.size()) return bad("column count", D, s.n, (long long)want.size());
  int c = 0;
  for (int32_t x : want) {
    if (s.col[c] != x || s.slot_of(x) != c) return bad("column order", D, c, x);
    ++c;
  }
  for (int x = 0; x < D; ++x)
    if (!want.count(x) && s.slot_of(x) != -1) return bad("a column without a derivative has a slot", D, x, s.slot_of(x));
}

static void check_tiles(int64_t Np, int dc, int64_t M) {
  const int64_t mt_max = slope_predict_rows_max(Np);
  if (mt_max % SLOPE_TILE || mt_max < SLOPE_TILE || mt_max > 32768) return bad("prediction tile", Np, dc, mt_max);
  if (mt_max > SLOPE_TILE && (double)mt_max * (double)Np * 8.0 > 8.0 * 1024 * 1024 * 1024) return bad("prediction tile over 8 GiB", Np, dc, mt_max);
  const int64_t mt = slope_tile_rows(mt_max, dc);
  if (mt % SLOPE_TILE || mt < SLOPE_TILE) return bad("slope tile", Np, dc, mt);
  if (mt_max >= (int64_t)dc * SLOPE_TILE && (int64_t)dc * mt > mt_max) return bad("stacked blocks exceed the prediction's tile", Np, dc, mt);
  if (mt > SLOPE_TILE && (int64_t)dc * (mt + SLOPE_TILE) <= mt_max) return bad("slope tile smaller than it could be", Np, dc, mt);
  // the M-tiles cover 0 .. M once, each within the tile
  int64_t covered = 0;
  for (int64_t m0 = 0; m0 < M; m0 += mt) {
    const int64_t mc = std::min<int64_t>(mt, M - m0);
    const int64_t mpad = (mc + SLOPE_TILE - 1) / SLOPE_TILE * SLOPE_TILE;
    if (mc < 1 || mpad > mt || mpad < mc) return bad("M-tile", M, m0, mc);
    covered += mc;
  }
  if (covered != M) return bad("M-tiles do not cover M", M, covered, mt);
}

static void check_layout(int64_t mpad, int dc, int64_t Np) {
  const SlopeLayout lay{mpad, dc};
  if (lay.ldz() != (int64_t)dc * mpad || lay.ldz() % SLOPE_TILE) return bad("ldz", mpad, dc, lay.ldz());
  std::vector<unsigned char> hit((size_t)lay.doubles(Np), 0);
  for (int64_t n = 0; n < Np; ++n)
    for (int c = 0; c < dc; ++c)
      for (int64_t m = 0; m < mpad; ++m) {
        const int64_t at = lay.at(c, m, n);
        if (at < 0 || at >= lay.doubles(Np)) return bad("element outside the buffer", c, m, n);
        if (hit[(size_t)at]++) return bad("element written twice", c, m, n);
        if (lay.row(c, m) != m + (int64_t)c * mpad) return bad("row", c, m, n);
      }
  for (unsigned char h : hit)
    if (h != 1) return bad("element never written", mpad, dc, Np);
}

static void check_pairs(int dc) {
  // the packed triangle: every (d, e <= d) its own entry, behind the Dc means
  std::vector<int> seen((size_t)slope_entries(dc, true), 0);
  for (int d = 0; d < dc; ++d)
    for (int e = 0; e <= d; ++e) {
      const int q = dc + slope_tri(d, e);
      if (q < dc || q >= slope_entries(dc, true) || seen[(size_t)q]++) return bad("packed triangle", dc, d, e);
    }
  if (slope_entries(dc, false) != 2 * dc) return bad("entries without the covariance", dc, slope_entries(dc, false), 0);
  // the blocks: z -> (bi, bj <= bi) as the kernel decodes it; every pair in exactly one block
  const int nb = slope_col_blocks(dc);
  if (slope_pair_blocks(dc, true) != nb * (nb + 1) / 2 || slope_pair_blocks(dc, false) != nb) return bad("block count", dc, nb, 0);
  std::vector<int> pair((size_t)(dc * dc), 0);
  for (int z = 0; z < slope_pair_blocks(dc, true); ++z) {
    int bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= z) ++bi;
    const int bj = z - bi * (bi + 1) / 2;
    if (bj > bi || bi >= nb) return bad("block decode", dc, z, bi);
    for (int r = 0; r < SLOPE_BLK; ++r)
      for (int c = 0; c < SLOPE_BLK; ++c) {
        const int d = SLOPE_BLK * bi + r, e = SLOPE_BLK * bj + c;
        if (d < dc && e <= d) ++pair[(size_t)(d * dc + e)];
      }
  }
  for (int d = 0; d < dc; ++d)
    for (int e = 0; e <= d; ++e)
      if (pair[(size_t)(d * dc + e)] != 1) return bad("a pair is not in exactly one block", dc, d, e);
}

int main() {
  // term layouts: one term; an additive model's three terms over the same columns; terms over different columns; a column that
  // is continuous and linear; periodic terms name every column twice
  check_columns(3, {{0, 1, 2}}, {{}});
  check_columns(5, {{0, 1}, {0, 1}, {0, 1}}, {{1}, {1}, {1}});
  check_columns(6, {{4, 0}, {2}}, {{5}, {0}});
  check_columns(4, {{3, 3, 1, 1}}, {{}});
  check_columns(24, {{15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0}}, {{23, 22, 21, 20, 19, 18, 17, 16}});
  {
    SlopeColumns s;
    const int32_t neg[1] = {-1};
    if (slope_add_columns(s, neg, 1)) bad("a negative column was accepted", 0, 0, 0);
    std::vector<int32_t> many(SLOPE_MAX_COLS + 1);
    for (int i = 0; i <= SLOPE_MAX_COLS; ++i) many[(size_t)i] = i;
    SlopeColumns t;
    if (slope_add_columns(t, many.data(), (int)many.size()) || t.n != SLOPE_MAX_COLS) bad("a 25th column was accepted", t.n, 0, 0);
  }
  for (int64_t Np : {(int64_t)128, (int64_t)768, (int64_t)10112, (int64_t)50048, (int64_t)2000000, (int64_t)20000000})
    for (int dc : {1, 2, 3, 4, 5, 8, 16, 24})
      for (int64_t M : {(int64_t)1, (int64_t)129, (int64_t)200, (int64_t)11010, (int64_t)100000}) check_tiles(Np, dc, M);
  if (slope_tile_rows(slope_predict_rows_max(768), 3) != 10880) bad("the N = 700, d = 3 tile", slope_tile_rows(slope_predict_rows_max(768), 3), 0, 0);
  for (int64_t mpad : {(int64_t)128, (int64_t)256, (int64_t)384})
    for (int dc : {1, 2, 3, 5, 16})
      for (int64_t Np : {(int64_t)128, (int64_t)256}) check_layout(mpad, dc, Np);
  for (int dc = 1; dc <= SLOPE_MAX_COLS; ++dc) check_pairs(dc);
  std::printf("slope_plan_check: %d failure%s\n", failures, failures == 1 ? "" : "s");
  return failures ? 1 : 0;
}
