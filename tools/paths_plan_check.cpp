// paths_plan_check.cpp -- the index arithmetic of the pathwise posterior draws (gumbi_amd/csrc/paths_plan.hpp: M-tiles and point
// tiles, draw blocks and the Sp padding, chunks of the contraction index N + F, the lane-to-pair map, the partial slots) as a
// stand-alone host program:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/paths_plan_check.cpp -o paths_plan_check
//   ./paths_plan_check
//
// The lane maps, the chunk ranges, the draw tiles and the partial offsets are free functions of that header which the kernels of
// pathwise.hpp call themselves (PATHS_HD), so what is replayed here is what the kernels index with.
// For a sweep of (N, F, M, S) -- S = 1, 16, 17, 512, M = 1, F no multiple of 4 among them -- it replays what the kernels index:
// every (point, draw) of a tile is written by exactly one (point tile, draw block, lane, register) per chunk, inside the buffer
// the plan sizes; every contraction index in [0, N) and [0, F) is generated exactly once over the chunks and the lanes of a
// step, and nothing at or beyond N or F is; the own-draw slots are covered once.  One line per failure; exit status 0 when all
// agree (tests/test_pathwise_cpu.py builds and runs it plain and under the sanitizers).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../gumbi_amd/csrc/paths_plan.hpp"

using namespace gmb;

static int failures = 0;

static bool bad(const char* what, int64_t N, int64_t F, int64_t M, int64_t S) {
  std::printf("FAIL %s at N=%lld F=%lld M=%lld S=%lld\n", what, (long long)N, (long long)F, (long long)M, (long long)S);
  ++failures;
  return false;
}

// the contraction index: chunks of length `chunk` cover [0, N) and [0, F) exactly once through the lanes' (step, k) pairs
static bool check_cut(const PathsPlan& pl, int64_t chunk, int64_t nchunk, int64_t N, int64_t F, int64_t M, int64_t S) {
  if (chunk < 1 || chunk % PATHS_UNIT || nchunk < 1 || (nchunk - 1) * chunk >= pl.total || nchunk * chunk < pl.total)
    return bad("chunk length / count", N, F, M, S);
  std::vector<uint8_t> tn((size_t)pl.N4, 0), tf((size_t)pl.F4, 0);
  for (int64_t c = 0; c < nchunk; ++c) {
    const PathsRange r = pl.range(chunk, c);
    if (r.na % PATHS_K || r.nb % PATHS_K || r.fa % PATHS_K || r.fb % PATHS_K) return bad("range not a multiple of the MFMA's k", N, F, M, S);
    if (r.na > r.nb || r.nb > pl.N4 || r.fa > r.fb || r.fb > pl.F4) return bad("range outside the padded index", N, F, M, S);
    if (r.nb - r.na + r.fb - r.fa < 1) return bad("empty chunk", N, F, M, S);
    for (int64_t n = r.na; n < r.nb; n += PATHS_K)
      for (int lane = 0; lane < 64; lane += 16) ++tn[(size_t)(n + paths_lane_k(lane))];
    for (int64_t f = r.fa; f < r.fb; f += PATHS_K)
      for (int lane = 0; lane < 64; lane += 16) ++tf[(size_t)(f + paths_lane_k(lane))];
  }
  for (int64_t n = 0; n < pl.N4; ++n)
    if (tn[(size_t)n] != 1) return bad("training index not covered exactly once", N, F, M, S);
  for (int64_t f = 0; f < pl.F4; ++f)
    if (tf[(size_t)f] != 1) return bad("feature index not covered exactly once", N, F, M, S);
  if (pl.N4 < N || pl.N4 >= N + PATHS_K || pl.F4 < F || pl.F4 >= F + PATHS_K) return bad("padding of N or F", N, F, M, S);
  return true;
}

static bool check(int64_t N, int64_t F, int64_t M, int64_t S) {
  PathsPlan pl;
  if (pl.make(N, F, M, S)) return bad("make refuses", N, F, M, S);
  // the Sp padding and the draw blocks
  if (pl.Sp % PATHS_DRAW_TILE || pl.Sp < S || pl.Sp >= S + PATHS_DRAW_TILE) return bad("Sp", N, F, M, S);
  if ((int64_t)pl.ndb * PATHS_DRAWS < pl.Sp || (int64_t)(pl.ndb - 1) * PATHS_DRAWS >= pl.Sp) return bad("draw blocks", N, F, M, S);
  int tiles = 0;
  for (int db = 0; db < pl.ndb; ++db) {
    const int nt = pl.draw_tiles(db);
    if (nt < 1 || nt > PATHS_DRAWS / PATHS_DRAW_TILE) return bad("accumulator tiles of a draw block", N, F, M, S);
    tiles += nt;
  }
  if (tiles * PATHS_DRAW_TILE != pl.Sp) return bad("accumulator tiles do not add up to Sp", N, F, M, S);
  // the lane maps: 64 lanes generate the 16 x 4 pairs of a step and hold the 16 x 16 results once each
  {
    int pair[16][4] = {}, res[16][16] = {};
    for (int lane = 0; lane < 64; ++lane) {
      ++pair[paths_lane_row(lane)][paths_lane_k(lane)];
      for (int r = 0; r < 4; ++r) ++res[paths_result_row(lane, r)][paths_result_col(lane)];
    }
    for (int i = 0; i < 16; ++i) {
      for (int k = 0; k < 4; ++k)
        if (pair[i][k] != 1) return bad("lane-to-pair map", N, F, M, S);
      for (int j = 0; j < 16; ++j)
        if (res[i][j] != 1) return bad("lane-to-result map", N, F, M, S);
    }
  }
  // the M-tiles
  if (pl.ntile < 1 || pl.mt % PATHS_ROWS) return bad("tile count / rows", N, F, M, S);
  int64_t next = 0;
  const double part_cap = pl.part_doubles(), own_cap = pl.own_part_doubles(3), out_cap = pl.out_doubles();
  for (int64_t t = 0; t < pl.ntile; ++t) {
    if (pl.ntile > 3 && t > 0 && t < pl.ntile - 1) {  // (full tiles are all alike: the first stands for them)
      next += PATHS_M_TILE;
      continue;
    }
    const PathsTile tl = pl.tile(t);
    if (tl.first != next || tl.mc < 1 || tl.mc > PATHS_M_TILE) return bad("tiles do not follow each other", N, F, M, S);
    next += tl.mc;
    if (tl.mpad % PATHS_ROWS || tl.mpad < tl.mc || tl.mpad > pl.mt) return bad("padded rows of a tile", N, F, M, S);
    if (tl.pt * PATHS_PTS < tl.mc || (tl.pt - 1) * PATHS_PTS >= tl.mc || tl.pt * PATHS_PTS > tl.mpad) return bad("point tiles", N, F, M, S);
    if ((double)pl.Sp * (double)tl.mpad > out_cap) return bad("results beyond their buffer", N, F, M, S);
    if (!check_cut(pl, tl.chunk, tl.nchunk, N, F, M, S) || !check_cut(pl, tl.own_chunk, tl.own_nchunk, N, F, M, S)) return false;
    if (tl.nchunk * tl.pt * pl.ndb >= PATHS_TARGET_WGS + tl.pt * pl.ndb) return bad("more workgroups than the target allows", N, F, M, S);
    // the slots of ONE chunk (the last: the largest offsets): every (draw < Sp, point < 16 pt) written once, inside the buffer
    const int64_t c = tl.nchunk - 1;
    const double cap = tl.nchunk > 1 ? part_cap : out_cap;
    const bool small = tl.pt < 64;  // the whole slot map for small tiles; for large ones three point tiles against the bounds
    std::vector<uint8_t> hit(small ? (size_t)(pl.Sp * tl.mpad) : 0, 0);
    const int64_t base = pl.part_at(tl, c, 0, 0);
    const int64_t pts[3] = {0, tl.pt / 2, tl.pt - 1};
    for (int db = 0; db < pl.ndb; ++db)
      for (int tt = 0; tt < pl.draw_tiles(db); ++tt)
        for (int64_t pi = 0; pi < (small ? tl.pt : 3); ++pi) {
          const int64_t p = small ? pi : pts[pi];
          for (int lane = 0; lane < 64; ++lane)
            for (int r = 0; r < 4; ++r) {
              const int64_t s = (int64_t)db * PATHS_DRAWS + tt * PATHS_DRAW_TILE + paths_result_col(lane);
              const int64_t m = p * PATHS_PTS + paths_result_row(lane, r);
              const int64_t at = pl.part_at(tl, c, s, m);
              if (s >= pl.Sp || m >= tl.mpad || at < 0 || (double)at >= cap) return bad("a result outside the partials", N, F, M, S);
              if (small && ++hit[(size_t)(at - base)] != 1) return bad("two lanes write one result", N, F, M, S);
            }
        }
    if (small)
      for (int64_t s = 0; s < pl.Sp; ++s)
        for (int64_t m = 0; m < tl.pt * PATHS_PTS; ++m)
          if (hit[(size_t)(s * tl.mpad + m)] != 1) return bad("a result nobody writes", N, F, M, S);
    // the own-draw slots: [chunk][accumulator][point], 64 points per workgroup
    if (tl.mpad % PATHS_OWN_PTS) return bad("own-draw point blocks", N, F, M, S);
    const int64_t last = pl.own_part_at(tl, tl.own_nchunk - 1, 3, 2, tl.mpad - 1);
    if ((double)last >= own_cap || pl.own_part_at(tl, 0, 3, 0, 0) != 0) return bad("own-draw partials beyond their buffer", N, F, M, S);
    if (pl.own_part_at(tl, 1, 3, 0, 0) - pl.own_part_at(tl, 0, 3, 2, tl.mpad - 1) != 1) return bad("own-draw slots overlap or leave a gap", N, F, M, S);
  }
  if (next != M) return bad("tiles do not cover M", N, F, M, S);
  // the dump says the same and respects its capacity
  const int64_t n = paths_plan_dump(N, F, M, S, 3, nullptr, 0);
  if (N >= 1 && n != PATHS_DUMP_HEADER + 8 * pl.ntile) return bad("dump size", N, F, M, S);
  if (N >= 1 && pl.ntile <= 64) {
    std::vector<int64_t> out((size_t)n + 1, -7);
    if (paths_plan_dump(N, F, M, S, 3, out.data(), n) != n || out[(size_t)n] != -7) return bad("dump writes past its values", N, F, M, S);
    if (out[0] != pl.Sp || out[1] != pl.ndb || out[4] != pl.mt || out[5] != pl.ntile) return bad("dump header", N, F, M, S);
    std::vector<int64_t> small(4, -7);
    if (paths_plan_dump(N, F, M, S, 3, small.data(), 3) != n || small[3] != -7) return bad("dump ignores its capacity", N, F, M, S);
  }
  return true;
}

int main() {
  const int64_t Ns[] = {0, 1, 3, 4, 63, 64, 65, 300, 1000, 10000};
  const int64_t Fs[] = {1, 3, 4, 64, 66, 1000, 2048, 16384};
  const int64_t Ms[] = {1, 15, 16, 17, 333, 2000, 65535, 65536, 65537, 1000000};
  const int64_t Ss[] = {1, 2, 15, 16, 17, 64, 65, 80, 511, 512};
  int64_t cases = 0;
  for (int64_t N : Ns)
    for (int64_t F : Fs)
      for (int64_t M : Ms)
        for (int64_t S : Ss) {
          check(N, F, M, S);
          ++cases;
        }
  // refusals
  PathsPlan pl;
  if (pl.make(10, 10, 10, 0) != 1 || pl.make(10, 10, 10, 513) != 1 || pl.make(10, 0, 10, 1) != 2 || pl.make(10, 16385, 10, 1) != 2 ||
      pl.make(10, 10, 0, 1) != 3 || pl.make(-1, 10, 10, 1) != 4 || paths_plan_dump(0, 10, 10, 1, 3, nullptr, 0) != -4)
    bad("refusal codes", 0, 0, 0, 0);
  std::printf("%lld cases, %d failures\n", (long long)cases, failures);
  return failures ? 1 : 0;
}
