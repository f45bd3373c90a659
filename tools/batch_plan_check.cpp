// batch_plan_check.cpp -- the index arithmetic of gmb_predict_batches (gumbi_amd/csrc/batch_plan.hpp: M-tiles cut on whole batches,
// the chunks of the contraction over the training points, the partial slots -- the very functions engine.hip calls before anything
// is launched) as a stand-alone program for the sanitizers.  No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/batch_plan_check.cpp -o /tmp/batch_plan_check
//   /tmp/batch_plan_check
//
// Driven over a grid of (N, B, q), sizes that must be refused included.  For every accepted plan: the tiles cover the batches once,
// in order, no batch straddles a tile, every tile fits a prediction's largest M-tile and the workspace the plan asks for; the
// chunks of a tile cover the training points once, in order, in multiples of the unit (so of the MFMA's k = 4), with no empty
// chunk; the wave-to-pair map of the contraction kernels (lane -> test index lane & 15, training point n + (lane >> 4)) touches
// every (point of the batch, training point) pair exactly once and reads no row beyond the tile's points; every (chunk, batch,
// accumulator) partial tile has its own q x q slot inside the doubles the plan asks for -- a buffer of that size is really
// allocated and written.  The dump (gmb_debug_batch_plan) says the same and respects its capacity.  One line per failure; exit
// status 0 when all agree (tests/test_predict_batches_cpu.py builds and runs it plain and under the sanitizers).
#include <cstdio>
#include <vector>

#include "../gumbi_amd/csrc/batch_plan.hpp"

using namespace gmb;

static int failures = 0;

static void bad(const char* what, long long n, long long b, long long q) {
  std::printf("FAIL %s (N = %lld, B = %lld, q = %lld)\n", what, n, b, q);
  ++failures;
}

static void check(int64_t N, int64_t B, int32_t q, int want) {
  const int64_t Np = batch_round_up(N > 0 ? N : 1, BATCH_TILE);
  BatchPlan pl;
  const int rc = pl.make(N, Np, B, q);
  if (rc != want) return bad("status of make", N, B, q);
  if (batch_plan_dump(N, Np, B, q, nullptr, 0) != (rc ? -rc : BATCH_DUMP_HEADER + 6 * pl.ntile)) return bad("dump size", N, B, q);
  if (rc) return;
  const int64_t mt_max = batch_tile_rows_max(Np);
  if (mt_max % BATCH_TILE || mt_max < BATCH_TILE || mt_max > 32768 || (mt_max > BATCH_TILE && (double)mt_max * Np * 8.0 > 8.0 * 1024 * 1024 * 1024))
    return bad("largest M-tile", N, B, q);
  if (pl.bt < 1 || pl.bt * q > mt_max || (pl.bt + 1) * q <= mt_max) return bad("batches of a full tile", N, B, q);
  if (pl.mt % BATCH_TILE || pl.mt > mt_max) return bad("workspace rows", N, B, q);
  const int nacc = 3;  // any accumulator count: the slots scale with it
  const double need = pl.part_doubles(nacc);
  int64_t next = 0;
  for (int64_t t = 0; t < pl.ntile; ++t) {
    const BatchTile tl = pl.tile(t);
    if (tl.first != next || tl.nb < 1 || tl.nb > pl.bt || tl.mc != tl.nb * q) return bad("tile extent", N, B, q);
    if (tl.mpad % BATCH_TILE || tl.mpad < tl.mc || tl.mpad - tl.mc >= BATCH_TILE || tl.mpad > pl.mt) return bad("tile padding", N, B, q);
    if (t + 1 < pl.ntile && tl.nb != pl.bt) return bad("a tile before the last is not full", N, B, q);
    next += tl.nb;
    // the chunks: multiples of the unit, in order, none empty, the grid within a launch's limits
    if (tl.chunk < BATCH_UNIT || tl.chunk % BATCH_UNIT || tl.nchunk < 1 || tl.nchunk > 65535) return bad("chunk length", N, B, q);
    if ((tl.nchunk - 1) * tl.chunk >= N || tl.nchunk * tl.chunk < N) return bad("chunks cover the training points", N, B, q);
    if ((double)tl.nchunk * (double)tl.nb > (double)pl.slots) return bad("more (chunk, batch) pairs than slots", N, B, q);
    if ((double)tl.nb * q * q > pl.cov_doubles() || (double)tl.nb * q * q * 4 > pl.dcov_doubles(4)) return bad("result blocks", N, B, q);
    // the lanes of the first and the last batch of small tiles: every (j, n) pair once, rows inside the tile's points
    if (N <= 1000) {
      for (int64_t b : {(int64_t)0, tl.nb - 1}) {
        std::vector<int> seen((size_t)(q * N), 0);
        for (int64_t c = 0; c < tl.nchunk; ++c) {
          const int64_t n0 = c * tl.chunk, n1 = n0 + tl.chunk < N ? n0 + tl.chunk : N;
          for (int64_t n = n0; n < n1; n += 4)
            for (int lane = 0; lane < 64; ++lane) {
              const int r16 = lane & 15, kq = lane >> 4;
              if (r16 >= q || n + kq >= n1) continue;
              const int64_t m = b * q + r16;
              if (m >= tl.mc) return bad("a lane reads a row beyond the tile's points", N, B, q);
              ++seen[(size_t)(r16 * N + n + kq)];
            }
        }
        for (int v : seen)
          if (v != 1) return bad("a (point, training point) pair touched no or two times", N, B, q);
      }
    }
    // the partial slots: allocated at the size the plan asks for, every (chunk, batch, accumulator) tile written once
    if (need <= 5.0e5) {
      std::vector<char> slot((size_t)need, 0);
      for (int64_t c = 0; c < tl.nchunk; ++c)
        for (int64_t b = 0; b < tl.nb; ++b)
          for (int a = 0; a < nacc; ++a) {
            const int64_t at = pl.part_at(tl, c, b, nacc, a);
            if (at < 0 || (double)(at + q * q) > need) return bad("a partial tile outside the buffer", N, B, q);
            for (int i = 0; i < q * q; ++i)
              if (slot[(size_t)(at + i)]++) return bad("two partial tiles share a slot", N, B, q);
          }
    }
  }
  if (next != B) return bad("batches covered", N, B, q);
  // the dump: header and tiles as above, and never more than `cap` values written
  const int64_t n = batch_plan_dump(N, Np, B, q, nullptr, 0);
  std::vector<int64_t> out((size_t)n + 1, -7);
  if (batch_plan_dump(N, Np, B, q, out.data(), n) != n || out[(size_t)n] != -7) return bad("dump writes past its values", N, B, q);
  if (out[0] != pl.bt || out[1] != pl.ntile || out[2] != pl.mt || out[3] != pl.slots || out[4] != BATCH_UNIT) return bad("dump header", N, B, q);
  const BatchTile last = pl.tile(pl.ntile - 1);
  const size_t lt = (size_t)(BATCH_DUMP_HEADER + 6 * (pl.ntile - 1));
  if (out[lt] != last.first || out[lt + 1] != last.nb || out[lt + 2] != last.mc || out[lt + 3] != last.mpad || out[lt + 4] != last.chunk ||
      out[lt + 5] != last.nchunk)
    return bad("dump tiles", N, B, q);
  std::vector<int64_t> small(4, -7);
  if (batch_plan_dump(N, Np, B, q, small.data(), 3) != n || small[3] != -7) return bad("dump ignores its capacity", N, B, q);
}

int main() {
  const int64_t ns[] = {1, 3, 63, 64, 65, 140, 300, 1000, 10000, 50000, 1000000};
  const int64_t bs[] = {1, 2, 5, 10, 77, 512, 1024, 2047, 2048, 2049, 6553, 6554, 6556, 32768, 32769, 100000};
  const int32_t qs[] = {1, 2, 3, 5, 8, 15, 16};
  int plans = 0;
  for (int64_t N : ns)
    for (int64_t B : bs)
      for (int32_t q : qs) {
        check(N, B, q, 0);
        ++plans;
      }
  // sizes that must be refused
  check(300, 10, 0, 1);
  check(300, 10, 17, 1);
  check(300, 10, -1, 1);
  check(300, 0, 8, 2);
  check(300, -5, 8, 2);
  check(0, 10, 8, 3);
  check(300, ((int64_t)1 << 40) / 16 + 1, 16, 4);
  {  // Np smaller than N, or no multiple of the tile
    BatchPlan pl;
    if (pl.make(300, 256, 10, 8) != 3 || pl.make(300, 300, 10, 8) != 3) bad("status of make for a bad Np", 300, 10, 8);
  }
  std::printf("%d plans checked, %d failures\n", plans + 8, failures);
  return failures ? 1 : 0;
}
