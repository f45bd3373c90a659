// append_layout_check.cpp -- the host-side index arithmetic of gmb_append / gmb_truncate (gumbi_amd/csrc/append_layout.hpp: the very
// header engine.hip computes its sizes, offsets and copy plan with) exercised on HOST buffers laid out like the factor, as a
// stand-alone program for the sanitizers.  No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/append_layout_check.cpp -o /tmp/append_layout_check
//   /tmp/append_layout_check
//
// For every (N_old, N_new) of the list -- the appends of tests/test_gpu_append.py and their truncations back -- it
//   * lays out an "old" buffer of exactly ld_old x Np_old doubles whose entries encode their own (row, column),
//   * allocates the new buffer of exactly elems_new() doubles, runs the re-layout's copy plan (append_copy_block) with memcpy,
//   * walks every region refactor_tail reads or writes in the new buffer (rebuilt rows, panel, corner, the y row),
//   * checks that the kept lower triangle arrived entry for entry and that nothing else of the panel / corner was copied over,
//   * checks the split-k rule on the corner's shape: slices are multiples of 16, none empty, together exactly [0, k), and the
//     tile enumeration visits every computed tile once.
// Any index outside a buffer is an AddressSanitizer report; the program prints one line per case and exits 0 when all agree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gumbi_amd/csrc/append_layout.hpp"

using namespace gmb;

static int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::printf("FAIL %s: ", #cond);   \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
      ++failures;                        \
    }                                    \
  } while (0)

static double code(int64_t r, int64_t c) { return (double)r + 1e6 * (double)c; }

static void check_splitk(int64_t mt, int64_t nt, int64_t k) {
  if (mt <= 0 || nt <= 0 || k <= 0) return;
  const int tiles = splitk_tile_count((int)mt, (int)nt, 1);
  std::vector<int> seen((size_t)(mt * nt), 0);
  for (int t = 0; t < tiles; ++t) {
    int tm = -1, tn = -1;
    splitk_decode_tile(t, (int)nt, 1, tm, tn);
    CHECK(tm >= 0 && tm < mt && tn >= tm && tn < nt, "tile %d -> (%d, %d) of %lld x %lld", t, tm, tn, (long long)mt, (long long)nt);
    if (tm >= 0 && tm < mt && tn >= 0 && tn < nt) ++seen[(size_t)(tm * nt + tn)];
  }
  for (int64_t tm = 0; tm < mt; ++tm)
    for (int64_t tn = 0; tn < nt; ++tn) CHECK(seen[(size_t)(tm * nt + tn)] == (tn >= tm ? 1 : 0), "tile (%lld, %lld) seen %d times", (long long)tm, (long long)tn, seen[(size_t)(tm * nt + tn)]);
  int len = 0;
  const int S = splitk_rule(tiles, k, &len);
  CHECK(S >= 1 && len > 0 && len % SPLITK_KT == 0, "S = %d, len = %d", S, len);
  CHECK((int64_t)(S - 1) * len < k && (int64_t)S * len >= k, "slices of %d do not tile k = %lld in %d", len, (long long)k, S);
  CHECK(splitk_pinned_len(k, S) == len, "the rule's own S must be a valid pin");
  // the workspace [tile][slice][128 * 128]: the last partial ends at its end
  std::vector<char> ws((size_t)tiles * S);  // one byte per partial stands for its 128 x 128 doubles
  for (int t = 0; t < tiles; ++t)
    for (int s = 0; s < S; ++s) ws[(size_t)t * S + s] = 1;
  CHECK(splitk_pinned_len(k, (int)(k / SPLITK_KT) + 1) == 0, "more slices than k-tiles must be refused");
}

static void run_case(int64_t N_old, int64_t N_new, int64_t pad, bool roomy) {
  const int64_t Np_old = al_round_up(N_old, AL_TILE), Nr_old = al_round_up(N_old + 1, AL_TILE), ld_old = Nr_old + pad;
  // `roomy`: the resident buffer already holds the new size (a truncation, or an append after one) -- no re-layout unless ld changes
  const int64_t cap_A = roomy ? std::max(ld_old * Np_old, (al_round_up(N_new + 1, AL_TILE) + pad) * al_round_up(N_new, AL_TILE)) : ld_old * Np_old;
  const AppendLayout a = append_layout(N_old, ld_old, N_new, cap_A);
  CHECK(a.Np_old == Np_old && a.Nr_old == Nr_old, "old sizes");
  CHECK(a.I0 * AL_TILE <= std::min(N_old, N_new) && (a.I0 + 1) * AL_TILE > std::min(N_old, N_new), "I0 = %lld", (long long)a.I0);
  std::vector<double> oldb((size_t)cap_A, -1.0);
  for (int64_t c = 0; c < Np_old; ++c)
    for (int64_t r = 0; r < Nr_old; ++r) oldb[(size_t)(r + c * ld_old)] = code(r, c);
  std::vector<double> fresh;
  double* nb = oldb.data();
  int64_t nb_elems = cap_A;
  if (a.relayout) {
    fresh.assign((size_t)a.elems_new(), -2.0);
    nb = fresh.data();
    nb_elems = a.elems_new();
    for (int64_t c = 0; c < a.I0; ++c) {
      const AppendCopy cp = append_copy_block(a, c);
      for (int64_t j = 0; j < cp.cols; ++j)  // (hipMemcpy2D: `cols` rows of the copy, `rows` contiguous doubles each)
        std::memcpy(nb + cp.dst + j * a.ld_new, oldb.data() + cp.src + j * a.ld_old, (size_t)cp.rows * sizeof(double));
    }
  }
  CHECK(nb_elems >= a.ld_new * a.Np_new, "the buffer in use holds the new layout");
  // the kept lower triangle: block columns [0, I0), rows from the block's diagonal to 128 I0
  for (int64_t c = 0; c < a.I0 * AL_TILE; ++c)
    for (int64_t r = c / AL_TILE * AL_TILE; r < a.I0 * AL_TILE; ++r)
      CHECK(nb[r + c * a.ld_new] == code(r, c), "kept entry (%lld, %lld)", (long long)r, (long long)c);
  // the regions refactor_tail works on
  const AppendRegions g = append_regions(a);
  CHECK(g.nct * AL_TILE == a.Np_new && g.nrt * AL_TILE == a.Nr_new && g.nrt >= g.nct && g.nrt <= g.nct + 1, "tile counts");
  CHECK(g.panel_row_tiles >= 1 && g.corner_mt >= 0 && g.corner_nt == g.panel_row_tiles, "corner shape");
  for (int64_t c = 0; c < g.corner_k; ++c)  // the panel: rebuilt, then solved in place
    for (int64_t r = 0; r < g.panel_row_tiles * AL_TILE; ++r) {
      if (a.relayout) CHECK(nb[g.panel_off + r + c * a.ld_new] == -2.0, "panel entry (%lld, %lld) was copied over", (long long)r, (long long)c);
      nb[g.panel_off + r + c * a.ld_new] = 3.0;
    }
  for (int64_t c = 0; c < g.corner_mt * AL_TILE; ++c)  // the corner's lower tiles: updated by the split-k product, then factored
    for (int64_t r = c / AL_TILE * AL_TILE; r < g.corner_nt * AL_TILE; ++r) nb[g.corner_off + r + c * a.ld_new] = 4.0;
  for (int64_t c = 0; c < a.N_new; ++c) nb[a.N_new + c * a.ld_new] = 5.0;  // the y row, where extract_v reads v
  CHECK(a.N_new < a.Nr_new && a.N_new + (a.N_new - 1) * a.ld_new < nb_elems, "the y row lies inside the buffer");
  // the kept triangle is untouched by all of that
  for (int64_t c = 0; c < a.I0 * AL_TILE; ++c)
    for (int64_t r = c / AL_TILE * AL_TILE; r < a.I0 * AL_TILE; ++r)
      CHECK(nb[r + c * a.ld_new] == code(r, c), "kept entry (%lld, %lld) after the update", (long long)r, (long long)c);
  check_splitk(g.corner_mt, g.corner_nt, g.corner_k);
  std::printf("N %5lld -> %5lld pad %lld%s: ld %5lld -> %5lld, Np %5lld -> %5lld, I0 %2lld, %s, corner %lld x %lld tiles over k = %lld\n",
              (long long)N_old, (long long)N_new, (long long)pad, roomy ? " roomy" : "", (long long)a.ld_old, (long long)a.ld_new,
              (long long)a.Np_old, (long long)a.Np_new, (long long)a.I0, a.relayout ? "re-laid" : "in place", (long long)g.corner_mt,
              (long long)g.corner_nt, (long long)g.corner_k);
}

int main() {
  const int64_t cases[][2] = {{100, 5}, {120, 20}, {300, 1}, {383, 1}, {384, 1}, {300, 200}, {1000, 16}, {4224, 3},
                              {126, 1}, {127, 1}, {128, 1}, {600, 10}, {200, 30}, {1, 1}, {1, 127}, {255, 257}};
  for (const auto& c : cases) {
    run_case(c[0], c[0] + c[1], 0, false);   // append
    run_case(c[0] + c[1], c[0], 0, false);   // truncate back
    run_case(c[0], c[0] + c[1], 0, true);    // append into a buffer that is large enough already
    run_case(c[0], c[0] + c[1], 8, false);   // a padded leading dimension (the tuning build's GMB_LD_PAD)
  }
  run_case(500, 250, 0, false);
  run_case(500, 128, 0, false);  // a whole number of blocks: no corner columns left
  run_case(500, 1, 0, false);
  // the headline shape's split: one tile over k = 49920, and the timing tool's k = 9984
  check_splitk(1, 1, 49920);
  check_splitk(1, 1, 9984);
  check_splitk(1, 2, 9984);
  check_splitk(2, 3, 2048);
  check_splitk(1, 1, 16);
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("all layouts agree\n");
  return 0;
}
