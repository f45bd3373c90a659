// paths_plan.hpp -- the index arithmetic of the pathwise posterior draws (gmb_paths_prepare / gmb_paths_eval /
// gmb_paths_eval_own): how M points are cut into M-tiles and those into point tiles of one MFMA tile, how S draws are padded and
// cut into draw blocks, how the contraction index -- the N training points, then the F random features -- is cut into chunks,
// which (point, contraction index) pair a lane generates, where a result lands, and what the calls' own buffers take.
//
// No HIP, no engine types and no other project header: tools/paths_plan_check.cpp runs this very header on the host.
#pragma once
#include <stdint.h>

namespace gmb {

constexpr int PATHS_MAX_S = 512;          // draws of one prepared state
constexpr int PATHS_MAX_F = 16384;        // random features of the prior draw
constexpr int PATHS_PTS = 16;             // points of one wave of paths_eval_kernel: the rows of v_mfma_f64_16x16x4_f64
constexpr int PATHS_DRAW_TILE = 16;       // draws of one accumulator tile: its columns; Sp is a multiple of this
constexpr int PATHS_DRAWS = 64;           // draws of a draw block: four accumulator tiles fed by every generated value
constexpr int PATHS_K = 4;                // contraction indices of one MFMA
constexpr int PATHS_UNIT = 64;            // chunk lengths are multiples of this (and so of PATHS_K)
constexpr int PATHS_TARGET_WGS = 2048;    // waves an evaluation launch aims at: two per SIMD of the 256 compute units
constexpr int PATHS_ROWS = 128;           // M-tiles are padded to this (the prepared points' stride)
constexpr int PATHS_M_TILE = 65536;       // points of a full M-tile: its results are Sp x 65536 doubles at most (256 MiB at S = 512)
constexpr int PATHS_OWN_PTS = 64;         // points of one workgroup of paths_own_kernel (a lane each)

// The pieces below are what paths_eval_kernel / paths_own_kernel index with as well (pathwise.hpp calls these very functions), so
// the check program and the kernels cannot drift apart.  PATHS_HD: callable from host and device under a HIP compiler.
#if defined(__HIPCC__) || defined(__HIP__)
#define PATHS_HD __attribute__((host)) __attribute__((device)) inline constexpr
#else
#define PATHS_HD inline constexpr
#endif

PATHS_HD int64_t paths_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// the (point of the tile, contraction index of the step) pair lane `lane` generates: the MFMA's m operand ...
PATHS_HD int paths_lane_row(int lane) { return lane & 15; }
PATHS_HD int paths_lane_k(int lane) { return lane >> 4; }
// ... and where register `reg` (0 .. 3) of its accumulator belongs: point (lane >> 4) + 4 reg of the tile, draw lane & 15 of the
// accumulator tile
PATHS_HD int paths_result_row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
PATHS_HD int paths_result_col(int lane) { return lane & 15; }

// one chunk of the contraction index: training points [na, nb) and features [fa, fb), all four multiples of PATHS_K (the ends
// may pass N and F by less than PATHS_K: such indices enter as zeros)
struct PathsRange {
  int64_t na, nb, fa, fb;
};
// chunk c of a cut of length `chunk` of the index [0, N4) (training points) followed by [N4, N4 + F4) (features)
PATHS_HD PathsRange paths_range(int64_t N4, int64_t F4, int64_t chunk, int64_t c) {
  const int64_t total = N4 + F4;
  const int64_t k0 = c * chunk, k1 = k0 + chunk < total ? k0 + chunk : total;
  return PathsRange{k0 < N4 ? k0 : N4, k1 < N4 ? k1 : N4, (k0 > N4 ? k0 : N4) - N4, (k1 > N4 ? k1 : N4) - N4};
}
// accumulator tiles of draw block db of Sp padded draws (1 .. 4)
PATHS_HD int paths_draw_tiles(int Sp, int db) {
  const int full = PATHS_DRAWS / PATHS_DRAW_TILE, left = Sp / PATHS_DRAW_TILE - db * full;
  return left < full ? left : full;
}
// the all-draws partials of a tile: [chunk][draw of Sp][point of mpad]; the own-draw partials: [chunk][accumulator of nacc][point]
PATHS_HD int64_t paths_part_at(int64_t Sp, int64_t mpad, int64_t c, int64_t s, int64_t m) { return (c * Sp + s) * mpad + m; }
PATHS_HD int64_t paths_own_part_at(int64_t nacc, int64_t mpad, int64_t c, int64_t acc, int64_t m) { return (c * nacc + acc) * mpad + m; }

// one M-tile: points first .. first + mc - 1 in mpad rows; pt point tiles of 16; nchunk chunks of `chunk` contraction indices for
// the all-draws kernel, own_nchunk of own_chunk for the own-draw kernel (64 points per workgroup)
struct PathsTile {
  int64_t first, mc, mpad, pt, chunk, nchunk, own_chunk, own_nchunk;
};

struct PathsPlan {
  int64_t N = 0, F = 0, M = 0;
  int32_t S = 0, Sp = 0, ndb = 0;  // draws; padded to 16; draw blocks of 64
  int64_t N4 = 0, F4 = 0, total = 0;  // the contraction index: [0, N4) training points, [N4, N4 + F4) features
  int64_t mt = 0;     // rows of the largest (first) tile, padded
  int64_t ntile = 0;

  // 0 = fine; 1: S outside 1 .. 512, 2: F outside 1 .. 16384, 3: M < 1 or beyond 2^40, 4: N < 0 or beyond 2^40
  // (N = 0: the features alone, what gmb_paths_prepare evaluates at the training points)
  int make(int64_t n, int64_t f, int64_t m, int64_t s) {
    *this = PathsPlan{};
    if (s < 1 || s > PATHS_MAX_S) return 1;
    if (f < 1 || f > PATHS_MAX_F) return 2;
    if (m < 1 || m > ((int64_t)1 << 40)) return 3;
    if (n < 0 || n > ((int64_t)1 << 40)) return 4;
    N = n, F = f, M = m, S = (int32_t)s;
    Sp = (int32_t)paths_round_up(s, PATHS_DRAW_TILE);
    ndb = (Sp + PATHS_DRAWS - 1) / PATHS_DRAWS;
    N4 = paths_round_up(n, PATHS_K);
    F4 = paths_round_up(f, PATHS_K);
    total = N4 + F4;
    const int64_t m0 = m < PATHS_M_TILE ? m : PATHS_M_TILE;
    mt = paths_round_up(m0, PATHS_ROWS);
    ntile = (m + PATHS_M_TILE - 1) / PATHS_M_TILE;
    return 0;
  }
  // accumulator tiles of draw block db (1 .. 4)
  int draw_tiles(int db) const { return paths_draw_tiles(Sp, db); }
  // chunk length for `wgs` workgroups per chunk: as long as possible while the grid keeps PATHS_TARGET_WGS workgroups
  void cut(int64_t wgs, int64_t* chunk, int64_t* nchunk) const {
    int64_t want = (PATHS_TARGET_WGS + wgs - 1) / wgs;
    const int64_t most = (total + PATHS_UNIT - 1) / PATHS_UNIT;
    want = want < 1 ? 1 : (want > most ? most : want);
    int64_t len = (total + want - 1) / want;
    len = paths_round_up(len, PATHS_UNIT);
    *chunk = len;
    *nchunk = (total + len - 1) / len;
  }
  PathsTile tile(int64_t t) const {
    PathsTile tl{};
    tl.first = t * PATHS_M_TILE;
    tl.mc = M - tl.first < PATHS_M_TILE ? M - tl.first : PATHS_M_TILE;
    tl.mpad = paths_round_up(tl.mc, PATHS_ROWS);
    tl.pt = (tl.mc + PATHS_PTS - 1) / PATHS_PTS;
    cut(tl.pt * ndb, &tl.chunk, &tl.nchunk);
    cut(tl.mpad / PATHS_OWN_PTS, &tl.own_chunk, &tl.own_nchunk);
    return tl;
  }
  // chunk c of a cut of length `chunk`
  PathsRange range(int64_t chunk, int64_t c) const { return paths_range(N4, F4, chunk, c); }
  // the all-draws partials of a tile: [chunk][draw of Sp][point of mpad]; a tile of ONE chunk writes its results directly
  int64_t part_at(const PathsTile& tl, int64_t c, int64_t s, int64_t m) const { return paths_part_at(Sp, tl.mpad, c, s, m); }
  double part_doubles_of(const PathsTile& tl) const { return tl.nchunk > 1 ? (double)tl.nchunk * Sp * (double)tl.mpad : 0.0; }
  // the own-draw partials: [chunk][accumulator of nacc][point of mpad]
  int64_t own_part_at(const PathsTile& tl, int64_t c, int64_t nacc, int64_t acc, int64_t m) const { return paths_own_part_at(nacc, tl.mpad, c, acc, m); }
  double own_part_doubles_of(const PathsTile& tl, int nacc) const { return (double)tl.own_nchunk * nacc * (double)tl.mpad; }
  // what the calls' buffers are sized for: the larger of the first and the last tile (the only two sizes there are)
  double part_doubles() const {
    const double a = part_doubles_of(tile(0)), b = part_doubles_of(tile(ntile - 1));
    return a > b ? a : b;
  }
  double own_part_doubles(int nacc) const {
    const double a = own_part_doubles_of(tile(0), nacc), b = own_part_doubles_of(tile(ntile - 1), nacc);
    return a > b ? a : b;
  }
  double out_doubles() const { return (double)Sp * (double)mt; }
};

// the plan as numbers (gmb_debug_paths_plan): 8 header values (Sp, ndb, N4, F4, mt, ntile, doubles of the all-draws partials,
// doubles of the own-draw partials for `nacc` accumulators), then 8 per tile (first, mc, mpad, pt, chunk, nchunk, own_chunk,
// own_nchunk).  Writes at most `cap` of them and returns how many there are; a refused request returns -(code of make), N < 1: -4
constexpr int PATHS_DUMP_HEADER = 8;
inline int64_t paths_plan_dump(int64_t N, int64_t F, int64_t M, int64_t S, int32_t nacc, int64_t* out, int64_t cap) {
  PathsPlan pl;
  const int bad = N < 1 ? 4 : pl.make(N, F, M, S);
  if (bad) return -(int64_t)bad;
  int64_t n = 0;
  auto put = [&](int64_t v) {
    if (out && n < cap) out[n] = v;
    ++n;
  };
  put(pl.Sp), put(pl.ndb), put(pl.N4), put(pl.F4), put(pl.mt), put(pl.ntile), put((int64_t)pl.part_doubles()), put((int64_t)pl.own_part_doubles(nacc));
  for (int64_t t = 0; t < pl.ntile; ++t) {
    const PathsTile tl = pl.tile(t);
    put(tl.first), put(tl.mc), put(tl.mpad), put(tl.pt), put(tl.chunk), put(tl.nchunk), put(tl.own_chunk), put(tl.own_nchunk);
  }
  return n;
}

}  // namespace gmb
