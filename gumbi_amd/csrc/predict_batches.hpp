// predict_batches.hpp -- the joint posterior of many SMALL batches of test points, and its derivative with respect to the batch's
// own coordinates: what a reparameterised Monte-Carlo acquisition (q-EI) needs for R restarts at once (the reference optimises its
// botorch acquisition by autograd: gumbi/regression/botorch/GP.py:652, `propose(q=..)`).
//
// Batch b = q <= 16 consecutive test points P_b.  With V = K(X*, X) L^-T and W = V L^-1 = K(X*, X) Sigma^-1 of an M-tile (test
// index fastest, as gmb_predict_with_grad leaves them):
//   C_b[j, l]            = k(x_j, x_l) - sum_n V_jn V_ln + jitter 1{j = l}
//   d C_b[j, l] / d x_j  = d_1 k(x_j, x_l) - sum_n W_ln d k(x_j, x_n) / d x_j          (l != j)
//   d C_b[j, j] / d x_j  = d k(x_j, x_j) / d x_j - 2 sum_n W_jn d k(x_j, x_n) / d x_j  (gmb_predict_with_grad's d sigma^2)
// per term, summed over the terms of an additive model.  The sums over the N training points are 16 x 16 x N products per batch:
//   Q[j, l]   = sum_n V_jn V_ln
//   T_c[j, l] = sum_n S_jn (u*_jc - u_nc) W_ln,   S_jn = eta^2 f'(r^2_jn) F_jn     per prepared column c
//   B_i[j, l] = sum_n F_jn xl_ni W_ln                                              per linear column i
// on v_mfma_f64_16x16x4_f64.  One wave owns one (batch, chunk of N).  Its A operand is one (j, n) pair per lane -- j = lane & 15,
// n = n0 + (lane >> 4) -- computed from direct scaled differences as predict_grad.hpp does (the expansion cancels where the
// gradient is small); its B operand is W (or V) at test index lane & 15 of the batch and the same n, so ONE load serves both
// roles in Q and every accumulator shares the B fragment.  Rows and columns >= q enter as zeros.  D comes back as
// row (A's index) = (lane >> 4) + 4 reg, column (B's index) = lane & 15.
//
// Every wave writes its q x q partial tiles; the finishing kernels add them in chunk order and apply predict_grad.hpp's finishing
// rules (2 inv_ls, the periodic (sin, cos) rule, tau for the linear sums), which are linear in the accumulators: the within-batch
// prior pair (j, l) enters as one more point with weight 1 (l != j) or 2 (l = j, where its stationary part vanishes).  No atomics:
// the same bits call after call.  Beyond V and W nothing of size M x N is written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_plan.hpp"
#include "covariance.hpp"

namespace gmb {

// ---- Q = V V^T per batch ---------------------------------------------------------------------------------------------------------
struct BatchGramArgs {
  const double* V;  // V[m + n * mpad]
  int64_t mpad, N;
  int64_t nb;       // batches of the tile: grid.x
  int64_t chunk;    // training points per chunk (a multiple of BATCH_UNIT): grid.y chunks
  int32_t q;
  double* part;     // [chunk][batch][q][q]
};

__global__ __launch_bounds__(64) void batch_gram_partial_kernel(BatchGramArgs a) {
  const int lane = threadIdx.x, r16 = lane & 15, kq = lane >> 4;
  const int64_t b = blockIdx.x;
  const int64_t n0 = (int64_t)blockIdx.y * a.chunk;
  const int64_t n1 = n0 + a.chunk < a.N ? n0 + a.chunk : a.N;  // columns >= N of V belong to no training point
  const bool row = r16 < a.q;
  const double* src = a.V + b * a.q + (row ? r16 : 0);  // row b q + r16 < mc <= mpad whenever it is read
  d4 acc[2] = {d4{0.0, 0.0, 0.0, 0.0}, d4{0.0, 0.0, 0.0, 0.0}};  // even and odd steps: two independent MFMA chains
  for (int64_t n = n0; n < n1; n += 8) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t nn = n + 4 * h + kq;
      const double v = row && nn < n1 ? src[nn * a.mpad] : 0.0;
      acc[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, acc[h], 0, 0, 0);
    }
  }
  double* out = a.part + ((int64_t)blockIdx.y * a.nb + b) * a.q * a.q;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = kq + 4 * r;
    if (j < a.q && row) out[j * a.q + r16] = acc[0][r] + acc[1][r];
  }
}

// C_b = diag(k**) - Q + jitter I: the chunks in chunk order, the lower triangle computed and mirrored (exactly symmetric).  The
// prior covariance of the pairs l != j is added per term by batch_prior_kernel.  One thread per (batch, j, l).
struct BatchCovFinishArgs {
  const double* part;
  int32_t nchunk, q;
  int64_t nb;
  const double* kss;  // k(x_m, x_m) summed over the terms (no noise), per point of the tile
  double jitter;
  double* cov;        // [batch][q][q]
};

__global__ __launch_bounds__(256) void batch_cov_finish_kernel(BatchCovFinishArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int qq = a.q * a.q;
  if (idx >= a.nb * qq) return;
  const int64_t b = idx / qq;
  const int rem = (int)(idx - b * qq), j = rem / a.q, l = rem - j * a.q;
  if (l > j) return;
  double s = 0.0;
  for (int c = 0; c < a.nchunk; ++c) s += a.part[((int64_t)c * a.nb + b) * qq + rem];
  double* C = a.cov + b * qq;
  if (l == j) {
    C[rem] = a.kss[b * a.q + j] - s + a.jitter;
  } else {
    C[rem] = -s;
    C[l * a.q + j] = -s;
  }
}

// what the two per-term kernels below read of a term and of the tile's prepared test points
struct BatchTermArgs {
  CovParams p;
  const double* txs;  // prepared test points of the tile: [column][mpad], columns >= nc are zero
  const double* txl;
  const int32_t* tcat;
  int64_t mpad, nb;
  int32_t q, nc_pad;
};

// F_jl: the product of the coregion table entries of two points of the tile
__device__ __forceinline__ double batch_pair_tables(const BatchTermArgs& a, int64_t mj, int64_t ml) {
  double F = 1.0;
  for (int t = 0; t < a.p.n_tab; ++t)
    F *= a.p.tabs[a.p.tab_off[t] + a.tcat[(int64_t)t * a.mpad + mj] * a.p.tab_levels[t] + a.tcat[(int64_t)t * a.mpad + ml]];
  return F;
}

// cov[b, j, l] += k_t(x_j, x_l) for l < j, mirrored: the direct form of cov_general_tile.  One thread per (batch, j, l).
template <int KIND>
__global__ __launch_bounds__(256) void batch_prior_kernel(BatchTermArgs a, double* cov) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int qq = a.q * a.q;
  if (idx >= a.nb * qq) return;
  const int64_t b = idx / qq;
  const int rem = (int)(idx - b * qq), j = rem / a.q, l = rem - j * a.q;
  if (l >= j) return;
  const int64_t mj = b * a.q + j, ml = b * a.q + l;
  double r2 = 0.0;
  for (int k = 0; k < a.nc_pad; ++k) {
    const double d = a.txs[(int64_t)k * a.mpad + mj] - a.txs[(int64_t)k * a.mpad + ml];
    r2 = fma(d, d, r2);
  }
  double v = a.p.eta2 * stationary<KIND>(r2);
  if (a.p.n_lin > 0) {
    double s = 0.0;
    for (int k = 0; k < a.p.n_lin; ++k) s = fma(a.txl[(int64_t)k * a.mpad + mj], a.txl[(int64_t)k * a.mpad + ml], s);
    v = fma(a.p.tau, s, v);
  }
  v *= batch_pair_tables(a, mj, ml);
  double* C = cov + b * qq;
  const double sum = C[rem] + v;
  C[rem] = sum;
  C[l * a.q + j] = sum;
}

// ---- T_c and the linear sums per batch ---------------------------------------------------------------------------------------------
struct BatchGradArgs {
  CovParams p;
  PointSet test;    // the tile's prepared points (npad = mpad)
  PointSet train;
  const double* W;  // K(X*, X) Sigma^-1: W[m + n * test.npad]
  int64_t nb, chunk;
  int32_t q;
  double* part;     // [chunk][batch][accumulator][q][q]: accumulators 0 .. NC-1 = T_c, NC .. NC + n_lin - 1 = the linear sums
};

template <int KIND, int NC, bool GEN>
__global__ __launch_bounds__(64) void batch_grad_partial_kernel(BatchGradArgs a) {
  constexpr int NL = GEN ? MAX_LIN : 0;
  const CovParams& p = a.p;
  const int lane = threadIdx.x, r16 = lane & 15, kq = lane >> 4;
  const int64_t b = blockIdx.x;
  const int64_t n0 = (int64_t)blockIdx.y * a.chunk;
  const int64_t n1 = n0 + a.chunk < a.train.n ? n0 + a.chunk : a.train.n;  // n0 < n1: the grid holds no empty chunk
  const bool row = r16 < a.q;
  const int64_t m = b * a.q + (row ? r16 : 0);  // a real point of the tile, read by every lane; lanes >= q contribute zeros

  double xi[NC];
  d4 acc[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    xi[k] = a.test.xs[(int64_t)k * a.test.npad + m];
    acc[k] = d4{0.0, 0.0, 0.0, 0.0};
  }
  d4 lin[NL > 0 ? NL : 1];
  int ci[MAX_TABS];
  (void)lin;
  (void)ci;
  if constexpr (GEN) {
#pragma unroll
    for (int l = 0; l < NL; ++l) lin[l] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < MAX_TABS; ++t) ci[t] = t < p.n_tab ? a.test.cat[(int64_t)t * a.test.npad + m] * p.tab_levels[t] + p.tab_off[t] : 0;
  }
  const double* wsrc = a.W + m;
  for (int64_t n = n0; n < n1; n += 4) {
    const bool ok = row && n + kq < n1;
    const int64_t nn = n + kq < n1 ? n + kq : n1 - 1;  // a real training point either way
    const double w = ok ? wsrc[nn * a.test.npad] : 0.0;
    double d[NC], r2 = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      d[k] = xi[k] - a.train.xs[(int64_t)k * a.train.npad + nn];
      r2 = fma(d[k], d[k], r2);
    }
    double g = ok ? p.eta2 * stationary_dr2<KIND>(r2) : 0.0;
    if constexpr (GEN) {
      double F = ok ? 1.0 : 0.0;
#pragma unroll
      for (int t = 0; t < MAX_TABS; ++t)
        if (t < p.n_tab) F *= p.tabs[ci[t] + a.train.cat[(int64_t)t * a.train.npad + nn]];
      g *= F;
#pragma unroll
      for (int l = 0; l < NL; ++l)
        if (l < p.n_lin)
          lin[l] = __builtin_amdgcn_mfma_f64_16x16x4f64(F * a.train.xl[(int64_t)l * a.train.npad + nn], w, lin[l], 0, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(g * d[k], w, acc[k], 0, 0, 0);
  }
  const int nacc = NC + p.n_lin, qq = a.q * a.q;
  double* out = a.part + ((int64_t)blockIdx.y * a.nb + b) * nacc * qq;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = kq + 4 * r;
    if (j < a.q && row) {
#pragma unroll
      for (int k = 0; k < NC; ++k) out[k * qq + j * a.q + r16] = acc[k][r];
      if constexpr (GEN) {
#pragma unroll
        for (int l = 0; l < NL; ++l)
          if (l < p.n_lin) out[(NC + l) * qq + j * a.q + r16] = lin[l][r];
      }
    }
  }
}

// dcov[b, j, l, :] += the term's d C_b[j, l] / d x_j: the prior pair's accumulators minus the chunks' (in chunk order), times 2 on
// the diagonal, through the finishing rules.  One thread per (batch, j, l).
struct BatchGradFinishArgs {
  BatchTermArgs t;
  const double* part;
  int32_t nchunk, nc, periodic, D;
  int32_t idx_cont[16];  // X column per prepared column
  double scale[16];      // stationary: 2 inv_ls per prepared column; periodic: 2 (2 pi / T_d) per DIMENSION d
  int32_t idx_lin[MAX_LIN];
  double* dcov;          // [batch][q][q][D], zeroed by the caller before the first term
};

template <int KIND>
__global__ __launch_bounds__(256) void batch_grad_finish_kernel(BatchGradFinishArgs a) {
  const BatchTermArgs& t = a.t;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int qq = t.q * t.q;
  if (idx >= t.nb * qq) return;
  const int64_t b = idx / qq;
  const int rem = (int)(idx - b * qq), j = rem / t.q, l = rem - j * t.q;
  const int64_t mj = b * t.q + j, ml = b * t.q + l;
  const int nacc = t.nc_pad + t.p.n_lin;
  const double wgt = l == j ? 2.0 : 1.0;
  const double F = batch_pair_tables(t, mj, ml);
  double S = 0.0;  // of the prior pair; on the diagonal its differences are zero
  if (l != j) {
    double r2 = 0.0;
    for (int k = 0; k < t.nc_pad; ++k) {
      const double d = t.txs[(int64_t)k * t.mpad + mj] - t.txs[(int64_t)k * t.mpad + ml];
      r2 = fma(d, d, r2);
    }
    S = t.p.eta2 * stationary_dr2<KIND>(r2) * F;
  }
  auto chunks = [&](int acc) {
    double s = 0.0;
    for (int c = 0; c < a.nchunk; ++c) s += a.part[(((int64_t)c * t.nb + b) * nacc + acc) * qq + rem];
    return s;
  };
  auto total = [&](int k) {  // accumulator k of the prepared columns
    const double d = t.txs[(int64_t)k * t.mpad + mj] - t.txs[(int64_t)k * t.mpad + ml];
    return wgt * (S * d - chunks(k));
  };
  double* g = a.dcov + idx * a.D;
  if (a.periodic) {
    for (int d = 0; 2 * d < a.nc; ++d) {
      const double us = t.txs[(int64_t)(2 * d) * t.mpad + mj], uc = t.txs[(int64_t)(2 * d + 1) * t.mpad + mj];
      g[a.idx_cont[2 * d]] += a.scale[d] * (total(2 * d) * uc - total(2 * d + 1) * us);
    }
  } else {
    for (int k = 0; k < a.nc; ++k) g[a.idx_cont[k]] += a.scale[k] * total(k);
  }
  for (int i = 0; i < t.p.n_lin; ++i)
    g[a.idx_lin[i]] += t.p.tau * wgt * (F * t.txl[(int64_t)i * t.mpad + ml] - chunks(t.nc_pad + i));
}

}  // namespace gmb
