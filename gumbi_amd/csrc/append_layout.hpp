// append_layout.hpp -- the HOST-side index arithmetic of gmb_append / gmb_truncate and of the split-k product, free of any HIP type
// so that it compiles into a plain C++ program as well (tools/append_layout_check.cpp runs it under AddressSanitizer and
// UndefinedBehaviorSanitizer on host buffers laid out like the factor): sizes of the bordered factor buffer, which block columns
// of a resident factor survive a change of N, where they sit before and after a re-layout, which regions the update touches;
// the tile enumeration and the slice rule of gemm_splitk.hpp.
#pragma once
#include <stdint.h>

#include <algorithm>

#ifdef __HIPCC__
#define GMB_HD __host__ __device__
#else
#define GMB_HD
#endif

namespace gmb {

constexpr int64_t AL_TILE = 128;  // (= TILE of gemm_f64.hpp)
constexpr int SPLITK_KT = 16;     // (= KT)

// The bordered factor buffer of N observations: Np columns (N up to 128), Nr rows (N + 1 up to 128: row N carries y), column-major
// with leading dimension ld = Nr + pad.
struct AppendLayout {
  int64_t N_old, Np_old, Nr_old, ld_old;
  int64_t N_new, Np_new, Nr_new, ld_new;
  int64_t I0;     // block columns [0, I0) of the old factor are kept: floor(min(N_old, N_new) / 128)
  bool relayout;  // the factor moves to a second buffer (leading dimension or capacity changed)
  int64_t elems_new() const { return ld_new * Np_new; }
};

inline int64_t al_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// `cap_A`: doubles the resident factor buffer holds
inline AppendLayout append_layout(int64_t N_old, int64_t ld_old, int64_t N_new, int64_t cap_A) {
  AppendLayout a{};
  a.N_old = N_old;
  a.Np_old = al_round_up(N_old, AL_TILE);
  a.Nr_old = al_round_up(N_old + 1, AL_TILE);
  a.ld_old = ld_old;
  a.N_new = N_new;
  a.Np_new = al_round_up(N_new, AL_TILE);
  a.Nr_new = al_round_up(N_new + 1, AL_TILE);
  a.ld_new = a.Nr_new + (ld_old - a.Nr_old);
  a.I0 = std::min(N_old, N_new) / AL_TILE;
  a.relayout = a.ld_new != a.ld_old || cap_A < a.ld_new * a.Np_new;
  return a;
}

// One 2-D copy of the re-layout: block column c < I0 keeps rows [128 c, 128 I0) -- `rows` contiguous doubles per column, 128 columns
struct AppendCopy {
  int64_t src, dst;  // element offsets of the block's first entry in the old / new buffer
  int64_t rows, cols;
};
inline AppendCopy append_copy_block(const AppendLayout& a, int64_t c) {
  return AppendCopy{c * AL_TILE * (a.ld_old + 1), c * AL_TILE * (a.ld_new + 1), (a.I0 - c) * AL_TILE, AL_TILE};
}

// The regions refactor_tail works on in the NEW buffer, as element offsets and tile counts
struct AppendRegions {
  int64_t nct, nrt;          // block columns / block rows of the new buffer
  int64_t panel_off;         // first entry of the rebuilt rows' panel (rows >= 128 I0, columns [0, 128 I0))
  int64_t panel_row_tiles;   // nrt - I0
  int64_t corner_off;        // first entry of the corner (rows and columns >= 128 I0)
  int64_t corner_mt, corner_nt, corner_k;  // its column tiles, row tiles and the contraction length 128 I0
};
inline AppendRegions append_regions(const AppendLayout& a) {
  AppendRegions r{};
  r.nct = a.Np_new / AL_TILE;
  r.nrt = a.Nr_new / AL_TILE;
  r.panel_off = a.I0 * AL_TILE;
  r.panel_row_tiles = r.nrt - a.I0;
  r.corner_off = a.I0 * AL_TILE * (a.ld_new + 1);
  r.corner_mt = r.nct - a.I0;
  r.corner_nt = r.nrt - a.I0;
  r.corner_k = a.I0 * AL_TILE;
  return r;
}

// ---- the split-k product's enumeration and slice rule (gemm_splitk.hpp) -----------------------------------------------------------
// computed tiles, enumerated m-tile by m-tile (tn ascending inside): with tri, m-tile tm holds the n-tiles tm .. nt - 1
GMB_HD inline int splitk_tile_count(int mt, int nt, int tri) {  // saturates at INT32_MAX (callers bound it by 65535)
  int64_t n = 0;
  if (!tri) n = (int64_t)mt * nt;
  else {
    const int64_t q = mt < nt ? mt : nt;  // m-tiles that hold tiles: tm < min(mt, nt), each nt - tm
    n = q * nt - q * (q - 1) / 2;
  }
  return n > 0x7fffffff ? 0x7fffffff : (int)n;
}
GMB_HD inline void splitk_decode_tile(int t, int nt, int tri, int& tm, int& tn) {
  if (!tri) {
    tm = t / nt;
    tn = t - tm * nt;
    return;
  }
  tm = 0;
  while (t >= nt - tm) {
    t -= nt - tm;
    ++tm;
  }
  tn = tm + t;
}

// corners of at most this many tiles always take the split-k pair (S = 1 included: the degenerate shapes' path); larger ones only
// when the rule finds more than one slice for them
constexpr int SPLITK_FEW_TILES = 8;

// The split: about one workgroup per compute unit of the 256-CU part in flight (the upper end of "half to one": these launches
// stand alone on the chip), slices of at least 256 in k (below that the partial's 128 KiB write and the prologue outweigh the
// contraction), every slice a multiple of KT.  A function of (tiles, k) only.  *len receives the slice length.
inline int splitk_rule(long long tiles, int64_t k, int* len) {
  const int64_t units = k / SPLITK_KT;
  int64_t S = tiles > 0 ? 256 / tiles : 1;
  S = std::min<int64_t>(S, k / 256);
  S = std::max<int64_t>(S, 1);
  const int64_t l = (units + S - 1) / S * SPLITK_KT;
  if (len) *len = (int)l;
  return (int)((k + l - 1) / l);
}
// a pinned S: the slice length it implies, or 0 when a slice would be empty
inline int splitk_pinned_len(int64_t k, int S) {
  if (S < 1) return 0;
  const int64_t units = k / SPLITK_KT;
  const int64_t l = (units + S - 1) / S * SPLITK_KT;
  if (l <= 0 || (int64_t)(S - 1) * l >= k) return 0;
  return (int)l;
}


}  // namespace gmb
