// laplace_plan.hpp -- the index arithmetic of the Laplace path: how the lower triangle of an N x N matrix is cut into
// 128 x 128 tiles for the symmetric matrix-vector product, which workspace slot each tile writes its two partial vectors to, which
// slots the second launch adds for a block row and in what order, and how many partial sets the likelihood pass leaves behind.
//
// No HIP, no engine types and no other project header: tools/laplace_plan_check.cpp runs this very header on the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LAP_HOST_DEVICE __host__ __device__
#else
#define LAP_HOST_DEVICE
#endif

namespace gmb {

constexpr int LAP_TILE = 128;               // the tile of the covariance build and of the Cholesky
constexpr int LAP_SLOT = 2 * LAP_TILE;      // doubles per slot: the tile's row part (tile v_J -> out_I), then its column part (tile^T v_I -> out_J)
constexpr int LAP_LIK_BLOCK = 256;          // observations per workgroup of the likelihood pass
constexpr int LAP_LIK_SUMS = 6;             // its partial set: sum log p | sum a f | max |f_new - f| | max |f_new| | labels off {0, 1} | non-finite f
constexpr int LAP_VECTORS = 16;             // vectors of Np doubles the state keeps (laplace.hpp names them)
constexpr int64_t LAP_MAX_N = (int64_t)1 << 22;  // block rows stay below 2^15, slots below 2^30

// the slot of tile (I, J), J <= I: the lower triangle row by row
LAP_HOST_DEVICE inline int64_t lap_slot(int64_t I, int64_t J) { return I * (I + 1) / 2 + J; }

// Block row R of the product adds nt parts in this order: the row parts of the tiles (R, 0) .. (R, R), then the column parts of
// the tiles (R, R) .. (nt - 1, R).  The diagonal tile's column part holds its strictly lower elements only, so it counts twice
// in the list and each element of the matrix once.  Term q of block row R: where it lies in the workspace (in doubles).
LAP_HOST_DEVICE inline int64_t lap_term_offset(int64_t R, int64_t q) {
  return q <= R ? lap_slot(R, q) * LAP_SLOT : lap_slot(q - 1, R) * LAP_SLOT + LAP_TILE;
}
LAP_HOST_DEVICE inline int64_t lap_terms(int64_t nt) { return nt + 1; }

struct LaplacePlan {
  int64_t N = 0, Np = 0, Nr = 0;
  int64_t nt = 0;          // block rows
  int64_t slots = 0;       // tiles of the lower triangle = workspace slots
  int64_t lik_blocks = 0;  // partial sets of the likelihood pass

  // 0 = fine; 1: N < 1, 2: N > LAP_MAX_N
  int make(int64_t n) {
    *this = LaplacePlan{};
    if (n < 1) return 1;
    if (n > LAP_MAX_N) return 2;
    N = n;
    Np = (n + LAP_TILE - 1) / LAP_TILE * LAP_TILE;
    Nr = (n + 1 + LAP_TILE - 1) / LAP_TILE * LAP_TILE;
    nt = Np / LAP_TILE;
    slots = nt * (nt + 1) / 2;
    lik_blocks = Np / LAP_LIK_BLOCK + (Np % LAP_LIK_BLOCK ? 1 : 0);
    return 0;
  }
  double symv_doubles() const { return (double)slots * LAP_SLOT; }
  double lik_doubles() const { return (double)lik_blocks * LAP_LIK_SUMS; }
  double vector_doubles() const { return (double)LAP_VECTORS * (double)Np; }
  double sigma_doubles() const { return (double)Nr * (double)Np; }  // the resident Sigma: the bordered layout of the factor buffer
};

// the plan as numbers (gmb_debug_laplace_plan): LAP_DUMP_HEADER values, then per block row its nt + 1 term offsets
constexpr int LAP_DUMP_HEADER = 8;
inline int64_t laplace_plan_dump(const LaplacePlan& pl, double bytes_state, int64_t* out, int64_t cap) {
  int64_t n = 0;
  auto put = [&](int64_t v) {
    if (out && n < cap) out[n] = v;
    ++n;
  };
  put(pl.Np), put(pl.Nr), put(pl.nt), put(pl.slots), put(pl.lik_blocks), put(LAP_SLOT), put(LAP_LIK_SUMS), put((int64_t)bytes_state);
  for (int64_t R = 0; R < pl.nt; ++R)
    for (int64_t q = 0; q < lap_terms(pl.nt); ++q) put(lap_term_offset(R, q));
  return n;
}

}  // namespace gmb
