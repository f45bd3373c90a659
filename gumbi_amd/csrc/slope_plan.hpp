// slope_plan.hpp -- the index arithmetic of gmb_predict_slope: which model columns carry a derivative, how many
// test points one M-tile holds, and where the cross-covariance row of (column, point) sits in the stacked buffer.
//
// No HIP and no engine types: tools/slope_plan_check.cpp runs this very header on the host.
#pragma once
#include <stdint.h>

namespace gmb {

constexpr int SLOPE_MAX_COLS = 24;  // GMB_MAX_DIMS continuous + GMB_MAX_LIN linear columns: the most a model can differentiate
constexpr int SLOPE_TILE = 128;     // rows of the stacked buffer come in multiples of the GEMM tile

// The differentiable model columns: the union of the terms' continuous and linear X columns, each once, in ascending order of
// the column index.  slot[c] = X column of differentiable column c.
struct SlopeColumns {
  int n = 0;
  int32_t col[SLOPE_MAX_COLS] = {};
  // position of X column `x` in the list, or -1
  int slot_of(int x) const {
    for (int c = 0; c < n; ++c)
      if (col[c] == x) return c;
    return -1;
  }
};

// adds the X columns idx[0 .. cnt) (any order, repeats allowed) to the list; false when it would overflow or a column is negative
inline bool slope_add_columns(SlopeColumns& s, const int32_t* idx, int cnt) {
  for (int i = 0; i < cnt; ++i) {
    const int32_t x = idx[i];
    if (x < 0) return false;
    int at = 0;
    while (at < s.n && s.col[at] < x) ++at;
    if (at < s.n && s.col[at] == x) continue;
    if (s.n >= SLOPE_MAX_COLS) return false;
    for (int j = s.n; j > at; --j) s.col[j] = s.col[j - 1];
    s.col[at] = x;
    ++s.n;
  }
  return true;
}

// a prediction's largest M-tile behind Np padded training points: the solved cross-covariance stays within 8 GiB, at most 32768
// rows, at least one tile (engine.hip: predict_tile_rows asked for an unbounded M)
inline int64_t slope_predict_rows_max(int64_t Np) {
  int64_t mt_max = (int64_t)(8.0 * 1024 * 1024 * 1024 / 8.0 / (double)Np);
  mt_max = mt_max / SLOPE_TILE * SLOPE_TILE;
  if (mt_max > 32768) mt_max = 32768;
  return mt_max < SLOPE_TILE ? SLOPE_TILE : mt_max;
}

// test points per M-tile: Dc stacked blocks share that budget
inline int64_t slope_tile_rows(int64_t mt_max, int dc) {
  if (dc < 1) dc = 1;
  const int64_t mt = mt_max / dc / SLOPE_TILE * SLOPE_TILE;
  return mt < SLOPE_TILE ? SLOPE_TILE : mt;
}

// the stacked buffer of one M-tile: mpad rows per differentiable column, test index fastest
struct SlopeLayout {
  int64_t mpad;  // a multiple of SLOPE_TILE
  int dc;
  int64_t ldz() const { return (int64_t)dc * mpad; }
  int64_t row(int c, int64_t m) const { return m + (int64_t)c * mpad; }
  int64_t at(int c, int64_t m, int64_t n) const { return row(c, m) + n * ldz(); }
  int64_t doubles(int64_t Np) const { return ldz() * Np; }
};

// the packed lower triangle of the Dc x Dc Gram: entry (d, e), e <= d
constexpr int slope_tri(int d, int e) { return d * (d + 1) / 2 + e; }

// entries per test point and chunk of the reduction: Dc dots with v, then the triangle (with_cov) or the Dc squares
constexpr int slope_entries(int dc, bool with_cov) { return dc + (with_cov ? dc * (dc + 1) / 2 : dc); }

// The (d, e) pairs are reduced in blocks of SLOPE_BLK x SLOPE_BLK columns, one block per kernel instance: block index z ->
// (bi, bj), bj <= bi, row-major over the lower triangle of blocks.  Without the covariance only the diagonal blocks run.
constexpr int SLOPE_BLK = 4;
constexpr int slope_col_blocks(int dc) { return (dc + SLOPE_BLK - 1) / SLOPE_BLK; }
inline int slope_pair_blocks(int dc, bool with_cov) {
  const int nb = slope_col_blocks(dc);
  return with_cov ? nb * (nb + 1) / 2 : nb;
}

}  // namespace gmb
