// design_plan.hpp -- the index arithmetic of gmb_design_batch: how the stacked set P = [candidates; reference
// points] is cut into point tiles, where a point sits in a row of D, the column chunks of the step kernel, the layout of its
// partial sums and what all of it takes in bytes.
//
// No HIP, no engine types and no other project header: tools/design_plan_check.cpp runs this very header on the host.
#pragma once
#include <stdint.h>

namespace gmb {

constexpr int DESIGN_TILE = 128;         // point tiles and the rows of D come in multiples of the GEMM tile
constexpr int DESIGN_THREADS = 256;      // threads of a step workgroup
constexpr int DESIGN_CHUNK = 2048;       // columns of D one step workgroup owns: 256 threads x 4 pairs of doubles
constexpr int DESIGN_ROWS = 4;           // candidate rows one step workgroup owns (the pivot row and the weights stay in registers)
constexpr int DESIGN_PICK_THREADS = 1024;  // the one workgroup of the pick kernel

inline int64_t design_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// a prediction's largest M-tile behind Np padded training points: V stays within 8 GiB, at most 32768 rows, at least one tile
// (engine.hip: predict_tile_rows asked for an unbounded M)
inline int64_t design_tile_rows_max(int64_t Np) {
  int64_t mt = (int64_t)(8.0 * 1024 * 1024 * 1024 / 8.0 / (double)Np);
  mt = mt / DESIGN_TILE * DESIGN_TILE;
  if (mt > 32768) mt = 32768;
  return mt < DESIGN_TILE ? DESIGN_TILE : mt;
}

// one point tile: `count` points of the stacked set from stacked index `first` on (candidates: 0 .. M - 1, reference points:
// M .. M + R - 1), at columns col0 .. col0 + mpad - 1 of D
struct DesignTile {
  int64_t first, count, mpad, col0;
};

// The plan of one call.  A row of D (one candidate) holds the candidates at columns 0 .. M - 1, zeros up to Mc (M rounded up to a
// tile), the reference points at Mc .. Mc + R - 1 and zeros up to ld: every point tile starts on a tile boundary of the row, which
// is what the covariance build and the GEMM write.  The candidates are ONE tile, the first: their solved rows are the GEMM's
// second operand for every other tile, so a call whose candidates do not fit one M-tile of a prediction is refused.
struct DesignPlan {
  int64_t Np = 0, M = 0, R = 0;
  int64_t Mc = 0;      // padded candidates: rows of D and of dVc
  int64_t ld = 0;      // doubles per row of D
  int64_t mt_max = 0;  // a prediction's largest M-tile behind Np
  int64_t mt = 0;      // rows of the prediction workspace the call needs: its largest tile
  int64_t ntile = 0;
  int64_t nchunk = 0;  // column chunks of the step kernel: partial sums part[chunk * Mc + row]

  // 0 = fine; 1: M < 1, 2: R < 1, 3: Np is no positive multiple of the tile, 4: the candidates do not fit one M-tile,
  // 5: an index of the call would leave 31 bits (columns of a row, or the elements of D leave 2^53)
  int make(int64_t np, int64_t m, int64_t r) {
    *this = DesignPlan{};
    if (m < 1) return 1;
    if (r < 1) return 2;
    if (np < DESIGN_TILE || np % DESIGN_TILE) return 3;
    Np = np, M = m, R = r;
    mt_max = design_tile_rows_max(np);
    if (m > mt_max) return 4;
    if (r > ((int64_t)1 << 30)) return 5;
    Mc = design_round_up(m, DESIGN_TILE);
    ld = Mc + design_round_up(r, DESIGN_TILE);
    const int64_t rt = r < mt_max ? design_round_up(r, DESIGN_TILE) : mt_max;
    mt = Mc > rt ? Mc : rt;
    ntile = 1 + (r + mt_max - 1) / mt_max;
    nchunk = (ld + DESIGN_CHUNK - 1) / DESIGN_CHUNK;
    return 0;
  }
  // tile 0: the candidates; tile t >= 1: reference points (t - 1) mt_max ..
  DesignTile tile(int64_t t) const {
    if (t == 0) return DesignTile{0, M, Mc, 0};
    const int64_t r0 = (t - 1) * mt_max;
    const int64_t c = R - r0 < mt_max ? R - r0 : mt_max;
    return DesignTile{M + r0, c, design_round_up(c, DESIGN_TILE), Mc + r0};
  }
  // the column of D that holds stacked point p
  int64_t col(int64_t p) const { return p < M ? p : Mc + (p - M); }
  // columns [c0, c1) of chunk c
  int64_t chunk_begin(int64_t c) const { return c * DESIGN_CHUNK; }
  int64_t chunk_end(int64_t c) const { return (c + 1) * DESIGN_CHUNK < ld ? (c + 1) * DESIGN_CHUNK : ld; }
  int64_t part_at(int64_t chunk, int64_t row) const { return chunk * Mc + row; }
  // the results' staging, in doubles: gains (q), score0 (M), ivar0 (1), picks (q, as int64)
  static int64_t result_doubles(int64_t m, int64_t q) { return 2 * q + m + 1; }
  // bytes of the feature's own buffers (a prediction's workspace for `mt` rows comes on top), in double: a request that has to be
  // refused may not fit in int64_t
  double own_bytes(int d, int xs_rows, int max_lin, int max_tabs, int64_t q) const {
    const double mc = (double)Mc, l = (double)ld;
    return 8.0 * (mc * (double)Np + mc * l)                                    // dVc, D
           + 8.0 * mc * ((double)d + xs_rows + max_lin) + 4.0 * mc * max_tabs  // the candidates, raw and prepared
           + 8.0 * 3.0 * l                                                     // pivot row, weights, latent variances
           + 8.0 * (double)nchunk * mc + 8.0 * mc + 4.0 * mc                   // partial sums, noise, mask
           + 8.0 * (DESIGN_CTL_DOUBLES + (double)result_doubles(M, q));
  }
  static constexpr int DESIGN_CTL_DOUBLES = 4;  // 1 / s of the pick, the "stopped" mark, two spare
};

// the plan as numbers (gmb_debug_design_plan): 9 header values, 4 per point tile, 2 per column chunk.  Writes at most `cap` of them
// and returns how many there are; a refused request returns -(code of make)
constexpr int DESIGN_DUMP_HEADER = 9;
inline int64_t design_plan_dump(int64_t Np, int64_t M, int64_t R, int64_t* out, int64_t cap) {
  DesignPlan pl;
  const int bad = pl.make(Np, M, R);
  if (bad) return -(int64_t)bad;
  int64_t n = 0;
  auto put = [&](int64_t v) {
    if (out && n < cap) out[n] = v;
    ++n;
  };
  put(pl.Mc), put(pl.ld), put(pl.mt_max), put(pl.mt), put(pl.ntile), put(pl.nchunk), put(DESIGN_CHUNK), put(DESIGN_ROWS);
  put((int64_t)pl.own_bytes(1, 0, 0, 0, 0));
  for (int64_t t = 0; t < pl.ntile; ++t) {
    const DesignTile tl = pl.tile(t);
    put(tl.first), put(tl.count), put(tl.mpad), put(tl.col0);
  }
  for (int64_t c = 0; c < pl.nchunk; ++c) put(pl.chunk_begin(c)), put(pl.chunk_end(c));
  return n;
}

}  // namespace gmb
