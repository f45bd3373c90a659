// fitc_plan.hpp -- the index arithmetic of the sparse (FITC) path: how the N columns of X are cut into column tiles
// behind m inducing points, the padded sizes of the m x m matrices and of an m x tile block, and how many partial sums the
// reductions of a tile leave behind.
//
// No HIP, no engine types and no other project header: tools/fitc_plan_check.cpp runs this very header on the host.
#pragma once
#include <stdint.h>

namespace gmb {

constexpr int FITC_TILE = 128;                // blocks come in multiples of the GEMM tile
constexpr int64_t FITC_MAX_TILE_ROWS = 32768;  // columns of X per tile at most (a prediction's largest M-tile)
constexpr int64_t FITC_MAX_M = 16384;         // inducing points at most: three m x m matrices stay below 7 GB
constexpr int FITC_COL_BLOCK = 32;            // columns of X per workgroup of the column kernels: one set of partial sums each
constexpr int FITC_COL_SUMS = 3;              // ... sum log lambda, sum y^2 / lambda, sum d
constexpr int FITC_DERIV_SUMS = 17;           // per workgroup of the derivative reduction: 16 lengthscale slots + eta
// bytes one m x tile block may take (there are four of them): the tile shrinks below FITC_MAX_TILE_ROWS only beyond m ~ 8000
constexpr double FITC_BLOCK_BYTES = 2147483648.0;

inline int64_t fitc_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// one column tile: columns [first, first + count) of X, padded to tpad
struct FitcTile {
  int64_t first, count, tpad;
};

struct FitcPlan {
  int64_t N = 0, m = 0;
  int64_t Np = 0;         // N rounded up to a tile: the length of the per-column vectors (lambda, alpha, d)
  int64_t mp = 0, mr = 0;  // m rounded up; m + 1 rounded up: the bordered layout of the Cholesky's routines (row m = the border)
  int64_t tile_rows = 0;  // columns of X per tile
  int64_t tmax = 0;       // ... of the widest tile of THIS N: rows of the block workspaces
  int64_t ntile = 0;

  // 0 = fine; 1: N < 1, 2: m < 1, 3: m > FITC_MAX_M, 4: N beyond 2^40
  int make(int64_t n, int64_t m_) {
    *this = FitcPlan{};
    if (n < 1) return 1;
    if (m_ < 1) return 2;
    if (m_ > FITC_MAX_M) return 3;
    if (n > ((int64_t)1 << 40)) return 4;
    N = n, m = m_;
    Np = fitc_round_up(n, FITC_TILE);
    mp = fitc_round_up(m_, FITC_TILE);
    mr = fitc_round_up(m_ + 1, FITC_TILE);
    int64_t t = (int64_t)(FITC_BLOCK_BYTES / 8.0 / (double)mr) / FITC_TILE * FITC_TILE;
    if (t > FITC_MAX_TILE_ROWS) t = FITC_MAX_TILE_ROWS;
    if (t < FITC_TILE) t = FITC_TILE;
    tile_rows = t;
    tmax = Np < t ? Np : t;
    ntile = (n + t - 1) / t;
    return 0;
  }
  FitcTile tile(int64_t t) const {
    const int64_t first = t * tile_rows;
    const int64_t c = N - first < tile_rows ? N - first : tile_rows;
    return FitcTile{first, c, fitc_round_up(c, FITC_TILE)};
  }
  // rows of a prediction's M-tile: the evaluation's tile rule for the test points
  int64_t predict_rows(int64_t M) const {
    const int64_t mpad = fitc_round_up(M, FITC_TILE);
    return mpad < tile_rows ? mpad : tile_rows;
  }
  // partial-sum sets of the column kernels over all of X (tiles start on multiples of FITC_TILE, so the blocks of 32 never straddle)
  int64_t col_blocks() const { return Np / FITC_COL_BLOCK; }
  // workgroups of the widest derivative reduction: a tile against Z, or Z against Z
  int64_t deriv_blocks() const {
    const int64_t a = (tmax / FITC_TILE) * (mp / FITC_TILE), b = (mp / FITC_TILE) * (mp / FITC_TILE);
    return a > b ? a : b;
  }
};

// the plan as numbers (gmb_debug_fitc_plan): FITC_DUMP_HEADER values, then (first, count, padded count) per tile.  `bytes_*`: what
// the buffer list of an evaluation with gradient takes for one continuous column (engine.hip fills them from workspaces.hpp).
constexpr int FITC_DUMP_HEADER = 10;
inline int64_t fitc_plan_dump(const FitcPlan& pl, double bytes_fixed, double bytes_blocks, double bytes_columns, int64_t* out, int64_t cap) {
  int64_t n = 0;
  auto put = [&](int64_t v) {
    if (out && n < cap) out[n] = v;
    ++n;
  };
  put(pl.Np), put(pl.mp), put(pl.mr), put(pl.tile_rows), put(pl.tmax), put(pl.ntile), put(pl.col_blocks());
  put((int64_t)bytes_fixed), put((int64_t)bytes_blocks), put((int64_t)bytes_columns);
  for (int64_t t = 0; t < pl.ntile; ++t) {
    const FitcTile tl = pl.tile(t);
    put(tl.first), put(tl.count), put(tl.tpad);
  }
  return n;
}

}  // namespace gmb
