// design_plan_check.cpp -- the index arithmetic of gmb_design_batch (gumbi_amd/csrc/design_plan.hpp: the point tiles, the layout of a
// row of D, the step kernel's column chunks and partial sums, the byte count -- the very functions engine.hip calls before anything
// is launched) as a stand-alone program for the sanitizers.  No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/design_plan_check.cpp -o /tmp/design_plan_check
//   /tmp/design_plan_check
//
// Driven over a grid of (Np, M, R), sizes that must be refused included.  For every accepted plan: the candidates are tile 0 and
// whole; every tile starts on a multiple of 128 of the row, holds at most a prediction's largest M-tile and fits the workspace the
// plan asks for; every stacked point has ONE column, inside its tile, and the columns of no point lie in the padding; the chunks
// cover the row once, in order, the step kernel's thread-to-column map (256 threads x 4 pairs, 512 columns apart) touches every
// column of a row exactly once -- a row is really allocated and counted -- and every (chunk, row) partial has its own slot.  The
// dump (gmb_debug_design_plan) says the same and respects its capacity.  One line per failure; exit status 0 when all agree
// (tests/test_design_cpu.py builds and runs it plain and under the sanitizers).
#include <cstdio>
#include <vector>

#include "../gumbi_amd/csrc/design_plan.hpp"

using namespace gmb;

static int failures = 0;

static void bad(const char* what, long long a, long long b, long long c) {
  std::printf("FAIL %s (Np = %lld, M = %lld, R = %lld)\n", what, a, b, c);
  ++failures;
}

static void check(int64_t Np, int64_t M, int64_t R, int want) {
  DesignPlan pl;
  const int rc = pl.make(Np, M, R);
  if (rc != want) return bad("status of make", Np, M, R);
  if (design_plan_dump(Np, M, R, nullptr, 0) != (rc ? -rc : DESIGN_DUMP_HEADER + 4 * pl.ntile + 2 * pl.nchunk)) return bad("dump size", Np, M, R);
  if (rc) return;
  const int64_t mt_max = design_tile_rows_max(Np);
  if (mt_max % DESIGN_TILE || mt_max < DESIGN_TILE || mt_max > 32768 || (mt_max > DESIGN_TILE && (double)mt_max * Np * 8.0 > 8.0 * 1024 * 1024 * 1024))
    return bad("largest M-tile", Np, M, R);
  if (pl.Mc % DESIGN_TILE || pl.Mc < M || pl.Mc - M >= DESIGN_TILE || pl.ld % DESIGN_TILE || pl.ld < pl.Mc + R || pl.ld % 2) return bad("padding", Np, M, R);
  // the tiles: candidates first and whole, then the reference points in order
  std::vector<int> owner((size_t)pl.ld, 0);  // how many points sit at a column
  int64_t next = 0;
  for (int64_t t = 0; t < pl.ntile; ++t) {
    const DesignTile tl = pl.tile(t);
    if (tl.first != next || tl.count < 1 || tl.mpad % DESIGN_TILE || tl.mpad < tl.count || tl.mpad - tl.count >= DESIGN_TILE) return bad("tile extent", Np, M, R);
    if (tl.col0 % DESIGN_TILE || tl.col0 + tl.mpad > pl.ld || tl.mpad > pl.mt || tl.mpad > mt_max) return bad("tile position", Np, M, R);
    if ((t == 0) != (tl.first == 0) || (t == 0 && (tl.count != M || tl.col0 != 0 || tl.mpad != pl.Mc))) return bad("candidate tile", Np, M, R);
    for (int64_t i = 0; i < tl.count; ++i) {
      const int64_t col = pl.col(tl.first + i);
      if (col != tl.col0 + i) return bad("column of a point", Np, M, R);
      ++owner[(size_t)col];
    }
    next += tl.count;
  }
  if (next != M + R) return bad("points covered", Np, M, R);
  for (int64_t c = 0; c < pl.ld; ++c) {
    const bool real = c < M || (c >= pl.Mc && c < pl.Mc + R);
    if (owner[(size_t)c] != (real ? 1 : 0)) return bad("a column with no or two points", Np, M, R);
  }
  // the chunks and the step kernel's map: workgroup `chunk`, thread tid, pair k -> columns chunk_begin + 2 tid + 512 k, + 1
  std::vector<int> touched((size_t)pl.ld, 0);
  int64_t at = 0;
  for (int64_t c = 0; c < pl.nchunk; ++c) {
    if (pl.chunk_begin(c) != at || pl.chunk_end(c) <= at || pl.chunk_end(c) - at > DESIGN_CHUNK) return bad("chunk extent", Np, M, R);
    at = pl.chunk_end(c);
    for (int tid = 0; tid < DESIGN_THREADS; ++tid)
      for (int k = 0; k < DESIGN_CHUNK / (2 * DESIGN_THREADS); ++k) {
        const int64_t col = pl.chunk_begin(c) + 2 * tid + (int64_t)k * 2 * DESIGN_THREADS;
        if (col >= pl.ld) continue;
        if (col + 1 >= pl.ld || col >= pl.chunk_end(c)) return bad("a pair straddles the end of the row or of its chunk", Np, M, R);
        ++touched[(size_t)col], ++touched[(size_t)col + 1];
      }
  }
  if (at != pl.ld) return bad("chunks cover the row", Np, M, R);
  for (int64_t c = 0; c < pl.ld; ++c)
    if (touched[(size_t)c] != 1) return bad("a column touched no or two times", Np, M, R);
  // the partial sums: every (chunk, row) its own slot of nchunk x Mc
  std::vector<char> slot((size_t)(pl.nchunk * pl.Mc), 0);
  for (int64_t c = 0; c < pl.nchunk; ++c)
    for (int64_t a = 0; a < M; ++a) {
      const int64_t s = pl.part_at(c, a);
      if (s < 0 || s >= pl.nchunk * pl.Mc || slot[(size_t)s]++) return bad("partial-sum slot", Np, M, R);
    }
  // bytes: D and the candidates' solved rows dominate and are counted exactly
  const double own = pl.own_bytes(4, 17, 8, 4, 8);
  const double big = 8.0 * ((double)pl.Mc * (double)Np + (double)pl.Mc * (double)pl.ld);
  if (!(own > big) || own > big + 8.0 * (double)pl.Mc * (40.0 + (double)pl.nchunk) + 24.0 * (double)pl.ld + 1024.0) return bad("bytes", Np, M, R);
  // the dump: header, tiles and chunks as above, and never more than `cap` values written
  const int64_t n = design_plan_dump(Np, M, R, nullptr, 0);
  std::vector<int64_t> out((size_t)n + 1, -7);
  if (design_plan_dump(Np, M, R, out.data(), n) != n || out[(size_t)n] != -7) return bad("dump writes past its values", Np, M, R);
  if (out[0] != pl.Mc || out[1] != pl.ld || out[4] != pl.ntile || out[5] != pl.nchunk || out[6] != DESIGN_CHUNK) return bad("dump header", Np, M, R);
  const DesignTile last = pl.tile(pl.ntile - 1);
  const size_t lt = (size_t)(DESIGN_DUMP_HEADER + 4 * (pl.ntile - 1));
  if (out[lt] != last.first || out[lt + 1] != last.count || out[lt + 2] != last.mpad || out[lt + 3] != last.col0) return bad("dump tiles", Np, M, R);
  if (out[(size_t)n - 1] != pl.ld) return bad("dump chunks", Np, M, R);
  std::vector<int64_t> small(4, -7);
  if (design_plan_dump(Np, M, R, small.data(), 3) != n || small[3] != -7) return bad("dump ignores its capacity", Np, M, R);
}

int main() {
  const int64_t nps[] = {128, 384, 768, 10112, 50048, 1000064, 20000000 / 128 * 128};
  const int64_t ms[] = {1, 5, 127, 128, 129, 130, 1024, 4097};
  const int64_t rs[] = {1, 127, 129, 2047, 2048, 2 * DESIGN_CHUNK + 1, 32768, 32769, 100000};
  int plans = 0;
  for (int64_t Np : nps)
    for (int64_t M : ms)
      for (int64_t R : rs) {
        const int want = M > design_tile_rows_max(Np) ? 4 : 0;
        check(Np, M, R, want);
        ++plans;
      }
  // sizes that must be refused
  check(768, 0, 10, 1);
  check(768, -3, 10, 1);
  check(768, 10, 0, 2);
  check(768, 10, -1, 2);
  check(0, 10, 10, 3);
  check(700, 10, 10, 3);
  check(768, 32769, 10, 4);
  check(1000064, 1025, 10, 4);  // 8 GiB / 8 MB per row = 1073 rows -> 1024
  check(768, 10, ((int64_t)1 << 30) + 1, 5);
  std::printf("%d plans checked, %d failures\n", plans + 9, failures);
  return failures ? 1 : 0;
}
