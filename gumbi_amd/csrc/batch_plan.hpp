// batch_plan.hpp -- the index arithmetic of gmb_predict_batches: how B batches of q points are cut into M-tiles of
// whole batches, how the N training points are cut into chunks of one wave's contraction, where a (chunk, batch, accumulator)
// partial tile sits, and what the call's own buffers take.
//
// No HIP, no engine types and no other project header: tools/batch_plan_check.cpp runs this very header on the host.
#pragma once
#include <stdint.h>

namespace gmb {

constexpr int BATCH_TILE = 128;           // M-tiles are padded to the GEMM tile, as a prediction's
constexpr int BATCH_MAX_Q = 16;           // points per batch: one 16 x 16 accumulator tile of v_mfma_f64_16x16x4_f64
constexpr int BATCH_UNIT = 64;            // chunk lengths are multiples of this (and so of the MFMA's k = 4)
constexpr int BATCH_TARGET_WAVES = 1024;  // waves a contraction launch aims at: one per SIMD of the 256 compute units

inline int64_t batch_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// a prediction's largest M-tile behind Np padded training points: V stays within 8 GiB, at most 32768 rows, at least one tile
// (engine.hip: predict_tile_rows asked for an unbounded M)
inline int64_t batch_tile_rows_max(int64_t Np) {
  int64_t mt = (int64_t)(8.0 * 1024 * 1024 * 1024 / 8.0 / (double)Np);
  mt = mt / BATCH_TILE * BATCH_TILE;
  if (mt > 32768) mt = 32768;
  return mt < BATCH_TILE ? BATCH_TILE : mt;
}

// one M-tile: batches first .. first + nb - 1, i.e. mc = nb q points in mpad rows of V; the contraction over the training points
// runs in nchunk chunks of `chunk` (the last one ragged), one wave per (batch, chunk)
struct BatchTile {
  int64_t first, nb, mc, mpad, chunk, nchunk;
};

struct BatchPlan {
  int64_t N = 0, Np = 0, B = 0;
  int32_t q = 0;
  int64_t bt = 0;     // batches of a full tile: a batch never straddles two tiles
  int64_t ntile = 0;
  int64_t mt = 0;     // rows of the prediction workspace the call needs: its largest (first) tile, padded
  int64_t slots = 0;  // (chunk, batch) pairs the partials are sized for: >= nchunk nb of every tile

  // 0 = fine; 1: q outside 1 .. 16, 2: B < 1, 3: N < 1 or Np no multiple of the tile that holds N, 4: B q leaves 2^40
  int make(int64_t n, int64_t np, int64_t b, int32_t qq) {
    *this = BatchPlan{};
    if (qq < 1 || qq > BATCH_MAX_Q) return 1;
    if (b < 1) return 2;
    if (n < 1 || np < n || np % BATCH_TILE) return 3;
    if (b > ((int64_t)1 << 40) / qq) return 4;
    N = n, Np = np, B = b, q = qq;
    bt = batch_tile_rows_max(np) / qq;
    ntile = (b + bt - 1) / bt;
    const int64_t nb0 = b < bt ? b : bt;
    mt = batch_round_up(nb0 * qq, BATCH_TILE);
    slots = BATCH_TARGET_WAVES + nb0;
    return 0;
  }
  // Chunk length of a tile of nb batches: as long as possible -- every chunk costs one set of partials and one more term of the
  // finishing sum -- while the grid keeps BATCH_TARGET_WAVES waves.  nchunk nb < BATCH_TARGET_WAVES + nb.
  BatchTile tile(int64_t t) const {
    BatchTile tl{};
    tl.first = t * bt;
    tl.nb = B - tl.first < bt ? B - tl.first : bt;
    tl.mc = tl.nb * q;
    tl.mpad = batch_round_up(tl.mc, BATCH_TILE);
    int64_t want = (BATCH_TARGET_WAVES + tl.nb - 1) / tl.nb;
    const int64_t most = (N + BATCH_UNIT - 1) / BATCH_UNIT;
    want = want < 1 ? 1 : (want > most ? most : want);
    int64_t len = (N + want - 1) / want;
    len = batch_round_up(len, BATCH_UNIT);
    tl.chunk = len;
    tl.nchunk = (N + len - 1) / len;
    return tl;
  }
  // the partial tile (q x q doubles, [j][l]) of accumulator `acc` of `nacc`, batch b of the tile's nb, chunk c
  int64_t part_at(const BatchTile& tl, int64_t c, int64_t b, int64_t nacc, int64_t acc) const {
    return ((c * tl.nb + b) * nacc + acc) * q * q;
  }
  // doubles of the partials for `nacc` accumulators per (chunk, batch)
  double part_doubles(int64_t nacc) const { return (double)slots * (double)nacc * q * q; }
  // doubles of the tile's results: the covariance blocks and their derivatives with respect to D columns
  double cov_doubles() const { return (double)(B < bt ? B : bt) * q * q; }
  double dcov_doubles(int D) const { return cov_doubles() * D; }
};

// the plan as numbers (gmb_debug_batch_plan): 5 header values (bt, ntile, mt, slots, BATCH_UNIT), then 6 per tile (first, nb, mc,
// mpad, chunk, nchunk).  Writes at most `cap` of them and returns how many there are; a refused request returns -(code of make)
constexpr int BATCH_DUMP_HEADER = 5;
inline int64_t batch_plan_dump(int64_t N, int64_t Np, int64_t B, int32_t q, int64_t* out, int64_t cap) {
  BatchPlan pl;
  const int bad = pl.make(N, Np, B, q);
  if (bad) return -(int64_t)bad;
  int64_t n = 0;
  auto put = [&](int64_t v) {
    if (out && n < cap) out[n] = v;
    ++n;
  };
  put(pl.bt), put(pl.ntile), put(pl.mt), put(pl.slots), put(BATCH_UNIT);
  for (int64_t t = 0; t < pl.ntile; ++t) {
    const BatchTile tl = pl.tile(t);
    put(tl.first), put(tl.nb), put(tl.mc), put(tl.mpad), put(tl.chunk), put(tl.nchunk);
  }
  return n;
}

}  // namespace gmb
