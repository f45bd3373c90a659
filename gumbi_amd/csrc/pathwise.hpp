// pathwise.hpp -- posterior FUNCTION draws by pathwise conditioning (Matheron's rule; the construction behind BoTorch's path
// samplers, the reference's second backend).  For draw s, with a prior draw from F random Fourier features,
//   f_s(x) = phi(x)^T w_s + k(x, X) a_s,   a_s = Sigma^-1 (y - Phi(X) w_s - d o eps_s),   d^2 = sigma^2 + jitter,
//   phi_f(x) = eta sqrt(2 / F) cos(omega_f^T u + b_f),   u = x / ls (the engine's prepared coordinates).
// gmb_paths_prepare forms A = [a_1 .. a_S] once (the prediction's two triangular passes with S right-hand sides); afterwards a
// draw is evaluated with no triangular pass: O(M (N + F)) fused arithmetic, and nothing of size M x N or M x M is written.
//
// paths_eval_kernel<KIND, NC>: Y = [K(X*, X) | Phi(X*)] [A ; w~] for ALL draws, on v_mfma_f64_16x16x4_f64.  One wave owns one
// (tile of 16 points, block of <= 64 draws, chunk of the contraction index).  Its m operand is one (point, index) pair per lane
// -- point lane & 15, index n0 + (lane >> 4) -- generated in registers: k(x*_i, x_n) from direct scaled differences (as kss_kernel
// and cov_general_tile do), or the feature cos(omega^T u + b).  Its n operand is the matching 4 x 16 fragment of A or of w~, both
// stored draw-fastest ([index][Sp]): four 128-byte runs per wave.  Every generated value feeds all (up to four) accumulator
// tiles of the draw block, so the exp and the differences are paid once per pair, not once per draw.  D comes back as point
// (lane >> 4) + 4 reg, draw lane & 15.  Points >= M and draws >= S enter as zeros.
//
// paths_own_kernel<KIND, NC>: point m on draw draw[m] ONLY, with the gradient over the continuous inputs -- what a Thompson
// search evaluates.  A vector kernel in the shape of predict_grad_partial_kernel: 64 points x 4 waves, the chunk's training
// points and features staged through LDS, the weight A[n Sp + draw[m]] where that kernel reads alpha[n].  It accumulates the
// value beside the gradient; a feature gives w~ cos(.) and -w~ sin(.) omega_c / ls_c (stored halved, so that the one finishing
// rule 2 inv_ls serves both parts).  The same stationary_dr2 and sqrt(r^2 + 1e-12) as the mean's gradient.
//
// Both write partials per chunk; the finishing kernels add them in chunk order.  No atomics: the same bits call after call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covariance.hpp"
#include "paths_plan.hpp"

namespace gmb {

struct PathsEvalArgs {
  const double* txs;  // prepared points of the tile: [column][tpad]
  int64_t tpad, mc;   // their stride; real points
  const double* xs;   // prepared training points: [column][npad]
  int64_t npad, N;
  const double* A;    // [row of >= N4][Sp], zeros beyond N and beyond S
  const double* wt;   // [feature of F4][Sp]: w eta sqrt(2 / F), zeros beyond F and beyond S
  const double* omega;  // [column of NC][F4], zeros beyond the real columns and beyond F
  const double* phase;  // [F4]
  int64_t F, F4, N4;
  int32_t Sp;
  double eta2;
  int64_t chunk;      // contraction indices per chunk: grid.z chunks
  double* part;       // [chunk][draw of Sp][point of mpad]
  int64_t mpad;
};

template <int KIND, int NC>
__global__ __launch_bounds__(64) void paths_eval_kernel(PathsEvalArgs a) {
  constexpr int NT = PATHS_DRAWS / PATHS_DRAW_TILE;
  const int lane = threadIdx.x, r16 = paths_lane_row(lane), kq = paths_lane_k(lane);  // the pair this lane generates (paths_plan.hpp)
  const int64_t m = (int64_t)blockIdx.x * PATHS_PTS + r16;
  const int db = blockIdx.y;
  const int nt = paths_draw_tiles(a.Sp, db);  // accumulator tiles of this draw block (uniform)
  const bool row = m < a.mc;
  const int64_t mr = row ? m : a.mc - 1;  // a real point either way
  const PathsRange rg = paths_range(a.N4, a.F4, a.chunk, blockIdx.z);
  const int64_t na = rg.na, nb = rg.nb, fa = rg.fa, fb = rg.fb;

  double xi[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) xi[k] = a.txs[(int64_t)k * a.tpad + mr];
  d4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  const int scol = db * PATHS_DRAWS + r16;  // draw of accumulator tile 0 this lane loads; tile t: + 16 t (< Sp for t < nt)

  for (int64_t n = na; n < nb; n += PATHS_K) {
    const int64_t nn = n + kq;          // < N4: a row of A
    const bool ok = row && nn < a.N;
    const int64_t nr = nn < a.N ? nn : a.N - 1;  // a real training point either way (na < nb only when N >= 1)
    double r2 = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const double d = xi[k] - a.xs[(int64_t)k * a.npad + nr];
      r2 = fma(d, d, r2);
    }
    const double v = ok ? a.eta2 * stationary<KIND>(r2) : 0.0;
    const double* b = a.A + nn * a.Sp + scol;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < nt) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(v, b[t * PATHS_DRAW_TILE], acc[t], 0, 0, 0);
  }
  for (int64_t f = fa; f < fb; f += PATHS_K) {
    const int64_t ff = f + kq;  // < F4: a row of wt, an entry of omega and phase
    double arg = a.phase[ff];
#pragma unroll
    for (int k = 0; k < NC; ++k) arg = fma(a.omega[(int64_t)k * a.F4 + ff], xi[k], arg);
    const double v = row && ff < a.F ? cos(arg) : 0.0;
    const double* b = a.wt + ff * a.Sp + scol;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < nt) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(v, b[t * PATHS_DRAW_TILE], acc[t], 0, 0, 0);
  }
  // point paths_result_row(lane, r) of the tile (< mpad: the grid covers ceil(mc / 16) tiles of a stride padded to 128), draw
  // scol + 16 t, where paths_result_col(lane) == r16 has gone into scol
  static_assert(paths_result_col(17) == paths_lane_row(17), "the draw a lane loads is the draw it holds");
  const int64_t p0 = (int64_t)blockIdx.x * PATHS_PTS;
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t < nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        a.part[paths_part_at(a.Sp, a.mpad, blockIdx.z, scol + t * PATHS_DRAW_TILE, p0 + paths_result_row(lane, r))] = acc[t][r];
    }
}

// out[s][m] = the chunks of part in chunk order.  One thread per (draw < S, point < mpad).
__global__ __launch_bounds__(256) void paths_eval_finish_kernel(const double* part, int32_t nchunk, int32_t Sp, int32_t S, int64_t mpad, double* out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)S * mpad) return;
  double s = 0.0;
  for (int c = 0; c < nchunk; ++c) s += part[paths_part_at(Sp, mpad, c, 0, idx)];
  out[idx] = s;
}

// ---- gmb_paths_prepare's own launches ---------------------------------------------------------------------------------------------
// R[s + n mrow] = y_n - P[s][n] - d eps[s][n] for the points n0 .. n0 + mc - 1 of one tile of the training points (P: the features
// alone, as paths_eval_kernel leaves them: [draw][point of mpad]); rows s >= S are zero.  One thread per (row of mrow, point).
__global__ __launch_bounds__(256) void paths_resid_kernel(const double* P, int64_t mpad, const double* y, const double* eps, int64_t N, int32_t S,
                                                          double d, int64_t n0, int64_t mc, double* R, int64_t mrow) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= mrow * mc) return;
  const int64_t j = idx / mrow, s = idx - j * mrow, n = n0 + j;
  R[s + n * mrow] = s < S ? y[n] - P[s * mpad + j] - d * eps[s * N + n] : 0.0;
}

// A[n][s] = W[s + n mrow] (the solved right-hand sides, draw index fastest as a prediction's test index) for n < N, s < S; zero
// elsewhere.  One thread per (row of `rows`, draw of Sp).
__global__ __launch_bounds__(256) void paths_store_a_kernel(const double* W, int64_t mrow, int64_t N, int64_t rows, int32_t S, int32_t Sp, double* A) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * Sp) return;
  const int64_t n = idx / Sp, s = idx - n * Sp;
  A[idx] = n < N && s < S ? W[s + n * mrow] : 0.0;
}

// ---- the own-draw kernel ------------------------------------------------------------------------------------------------------------
constexpr int PO_PIECE = 128;  // contraction indices staged in LDS at a time

struct PathsOwnArgs {
  const double* txs;  // prepared points of the tile: [column][mpad]
  int64_t mpad, mc;
  const int32_t* draw;  // per point, in [0, S) (checked by the caller); padding rows read draw 0
  const double* xs;
  int64_t npad, N;
  const double* A;
  const double* wt;
  const double* omega;
  const double* phase;
  int64_t F, F4, N4;
  int32_t Sp;
  double eta2;
  int64_t chunk;
  double* part;  // [chunk][accumulator][mpad]: 0 .. NC-1 = the gradient's sums per prepared column, NC = the value
};

template <int KIND, int NC>
__global__ __launch_bounds__(256) void paths_own_kernel(PathsOwnArgs a) {
  constexpr int NCS = (NC + 2) & ~1;  // row stride of a staged index: NC coordinates (or frequencies), the phase, padded to even
  constexpr int NACC = NC + 1;
  constexpr int STAGE = PO_PIECE * NCS;
  constexpr int RED = 3 * NACC * PATHS_OWN_PTS;
  __shared__ double smem[STAGE > RED ? STAGE : RED];
  double* sx = smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m = (int64_t)blockIdx.x * PATHS_OWN_PTS + lane;  // < mpad: the grid covers mpad / 64 blocks exactly
  const PathsRange rg = paths_range(a.N4, a.F4, a.chunk, blockIdx.y);
  int64_t na = rg.na, nb = rg.nb, fa = rg.fa, fb = rg.fb;
  nb = nb < a.N ? nb : a.N;  // indices in [N, N4) and [F, F4) belong to nothing
  na = na < nb ? na : nb;
  fb = fb < a.F ? fb : a.F;
  fa = fa < fb ? fa : fb;
  const int dm = m < a.mc ? a.draw[m] : 0;

  double xi[NC], acc[NC], val = 0.0;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    xi[k] = a.txs[(int64_t)k * a.mpad + m];
    acc[k] = 0.0;
  }
  for (int64_t q0 = na; q0 < nb; q0 += PO_PIECE) {
    const int cnt = (int)(nb - q0 < PO_PIECE ? nb - q0 : PO_PIECE);
    __syncthreads();  // the previous piece has been read
    for (int idx = tid; idx < NC * PO_PIECE; idx += 256) {
      const int k = idx / PO_PIECE, j = idx - k * PO_PIECE;
      if (j < cnt) sx[j * NCS + k] = a.xs[(int64_t)k * a.npad + q0 + j];
    }
    __syncthreads();
    const int j_lo = wave * (PO_PIECE / 4);
    const int j_hi = j_lo + PO_PIECE / 4 < cnt ? j_lo + PO_PIECE / 4 : cnt;
    const double* wcol = a.A + (q0 + j_lo) * a.Sp + dm;  // rows < N of A for every j read below
#pragma unroll 2
    for (int j = j_lo; j < j_hi; ++j) {
      const double* rowp = sx + j * NCS;
      double d[NC], r2 = 0.0;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        d[k] = xi[k] - rowp[k];
        r2 = fma(d[k], d[k], r2);
      }
      const double w = *wcol;
      wcol += a.Sp;
      val = fma(w * a.eta2, stationary<KIND>(r2), val);
      const double g = w * (a.eta2 * stationary_dr2<KIND>(r2));
#pragma unroll
      for (int k = 0; k < NC; ++k) acc[k] = fma(g, d[k], acc[k]);
    }
  }
  for (int64_t q0 = fa; q0 < fb; q0 += PO_PIECE) {
    const int cnt = (int)(fb - q0 < PO_PIECE ? fb - q0 : PO_PIECE);
    __syncthreads();
    for (int idx = tid; idx < (NC + 1) * PO_PIECE; idx += 256) {
      const int k = idx / PO_PIECE, j = idx - k * PO_PIECE;
      if (j < cnt) sx[j * NCS + k] = k < NC ? a.omega[(int64_t)k * a.F4 + q0 + j] : a.phase[q0 + j];
    }
    __syncthreads();
    const int j_lo = wave * (PO_PIECE / 4);
    const int j_hi = j_lo + PO_PIECE / 4 < cnt ? j_lo + PO_PIECE / 4 : cnt;
    const double* wcol = a.wt + (q0 + j_lo) * a.Sp + dm;
    for (int j = j_lo; j < j_hi; ++j) {
      const double* rowp = sx + j * NCS;
      double arg = rowp[NC];
#pragma unroll
      for (int k = 0; k < NC; ++k) arg = fma(rowp[k], xi[k], arg);
      double sn, cs;
      sincos(arg, &sn, &cs);
      const double w = *wcol;
      wcol += a.Sp;
      val = fma(w, cs, val);
      const double g = -0.5 * w * sn;  // halved: the finishing rule multiplies by 2 inv_ls
#pragma unroll
      for (int k = 0; k < NC; ++k) acc[k] = fma(g, rowp[k], acc[k]);
    }
  }

  // waves 1 .. 3 hand their accumulators to wave 0, which adds them in wave order and writes the chunk's partials
  double* red = smem;  // [3][NACC][64]
  __syncthreads();
  if (wave > 0) {
#pragma unroll
    for (int k = 0; k < NC; ++k) red[((wave - 1) * NACC + k) * PATHS_OWN_PTS + lane] = acc[k];
    red[((wave - 1) * NACC + NC) * PATHS_OWN_PTS + lane] = val;
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      double v = acc[k];
#pragma unroll
      for (int w = 0; w < 3; ++w) v += red[(w * NACC + k) * PATHS_OWN_PTS + lane];
      a.part[paths_own_part_at(NACC, a.mpad, blockIdx.y, k, m)] = v;
    }
    double v = val;
#pragma unroll
    for (int w = 0; w < 3; ++w) v += red[(w * NACC + NC) * PATHS_OWN_PTS + lane];
    a.part[paths_own_part_at(NACC, a.mpad, blockIdx.y, NC, m)] = v;
  }
}

// val[m] and grad[m][idx_cont[k]] = 2 inv_ls_k (sum of the chunks, in chunk order); the other columns of grad are the caller's
// zeros.  One thread per point.
struct PathsOwnFinishArgs {
  const double* part;
  int32_t nchunk, nc, nc_pad, D;
  int64_t mpad, mc;
  int32_t idx_cont[16];
  double scale[16];  // 2 inv_ls per prepared column
  double* val;
  double* grad;      // mc x D row-major, or null
};

__global__ __launch_bounds__(256) void paths_own_finish_kernel(PathsOwnFinishArgs a) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= a.mc) return;
  const int nacc = a.nc_pad + 1;
  auto total = [&](int acc) {
    double s = 0.0;
    for (int c = 0; c < a.nchunk; ++c) s += a.part[paths_own_part_at(nacc, a.mpad, c, acc, m)];
    return s;
  };
  a.val[m] = total(a.nc_pad);
  if (a.grad)
    for (int k = 0; k < a.nc; ++k) a.grad[m * a.D + a.idx_cont[k]] = a.scale[k] * total(k);
}

}  // namespace gmb
