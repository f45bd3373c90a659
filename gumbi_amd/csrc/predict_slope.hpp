// predict_slope.hpp -- the posterior of the slope d f / d x* at a test point: mean AND covariance.
//
// The derivative of a GP with a mean-square differentiable kernel is a GP.  For the selected terms S, with L, v = L^-1 y of the
// whole model and, per test point x* and differentiable model column d,
//   b_d[n]        = d k_S(x*, x_n) / d x*_d                                  row d of B
//   V_d           = b_d L^-T                                                  the prediction's solve, Dc rows per point
//   E[g_d]        = <V_d, v>                                                  (= d mu / d x*_d: what gmb_predict_grad returns)
//   Cov[g_d, g_e] = P_de - <V_d, V_e>
//   P_de          = delta_de sum_t F_t(x*, x*) [ -2 eta_t^2 f'_t(0) J_d^2 + tau_t 1{d linear in t} ]
// J_d^2 = 1 / ls_d^2 (stationary) or w_d^2 (2 pi / T_d)^2 (periodic, w_d the weight riding in the warped columns); f' =
// stationary_dr2 with its sqrt(r^2 + 1e-12).  b_d is predict_grad.hpp's per-pair expression with the finishing rule applied
// pair by pair instead of after the sum:
//   stationary        b_d = S 2 inv_ls_d (u*_d - u_nd),                         S = eta^2 f'(r^2) F_mn
//   periodic (1, 2)   b_d = S 2 (2 pi / T_d) ((u*_2d - u_n,2d) u*_(2d+1) - (u*_(2d+1) - u_n,2d+1) u*_2d)
//   linear            b_l += tau F_mn xl_nl
// Matern-1/2 and Exponential have no mean-square derivative (P would be infinite): gmb_predict_slope refuses them.
//
// slope_cross_cov_kernel WRITES b into the stacked buffer (slope_plan.hpp: row m + c mpad, column n, leading dimension
// ldz = Dc mpad), the prediction's own solve turns it into V, slope_gram_partial_kernel / slope_finish_kernel reduce V in two
// deterministic stages.  No atomics, every output written once: the same bits call after call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covariance.hpp"
#include "slope_plan.hpp"

namespace gmb {

// ---- the derivative cross-covariance ------------------------------------------------------------------------------------------
// A workgroup = 64 test points (one per lane) x 4 waves against ONE piece of 128 training points staged in LDS; wave w takes the
// piece's points 32 w .. 32 w + 31, so every LDS read is a broadcast and every store is a run of 64 consecutive doubles along m.
// The kernel is bound by those stores: Dc x mpad x Np doubles per M-tile.
constexpr int SC_PTS = 64;
constexpr int SC_PIECE = 128;

struct SlopeCovArgs {
  CovParams p;
  PointSet test;   // npad = mpad, a multiple of 128
  PointSet train;
  double* out;     // out[(m + c * mpad) + n * ldz]
  int64_t ldz;
  int32_t accumulate;  // a later term of an additive model: add to the real entries, leave the zeros alone
  int32_t periodic;
  int32_t nc;          // prepared continuous columns in use (periodic: 2 per dimension)
  int32_t dc;          // differentiable columns of the call
  int32_t slot[16];    // stationary: prepared column k -> differentiable column; periodic: DIMENSION d -> differentiable column
  double scale[16];    // stationary: 2 inv_ls_k; periodic: 2 (2 pi / T_d) per dimension
  int32_t slot_lin[MAX_LIN];
  int32_t lin_over[MAX_LIN];  // the linear column is one of this term's continuous columns too: its share is added
  uint32_t zero_slots;        // differentiable columns this (storing) term has no share in: written 0
};

template <int KIND, int NC, bool GEN>
__global__ __launch_bounds__(256) void slope_cross_cov_kernel(SlopeCovArgs a) {
  constexpr int NL = GEN ? MAX_LIN : 0;
  __shared__ double sx[SC_PIECE * NC];
  __shared__ double sl[GEN ? SC_PIECE * MAX_LIN : 1];
  __shared__ int32_t sc[GEN ? SC_PIECE * MAX_TABS : 1];
  (void)sl;
  (void)sc;
  const CovParams& p = a.p;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t mpad = a.test.npad;
  const int64_t m = (int64_t)blockIdx.x * SC_PTS + lane;  // < mpad: the grid covers mpad / 64 blocks exactly
  const int64_t q0 = (int64_t)blockIdx.y * SC_PIECE;      // < Np: the grid covers Np / 128 pieces exactly
  const int64_t left = a.train.n - q0;
  const int cnt = (int)(left < 0 ? 0 : (left < SC_PIECE ? left : SC_PIECE));  // columns >= N are written 0
  const bool real = m < a.test.n;                                             // ... and so are rows of no point

  double xi[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) xi[k] = a.test.xs[(int64_t)k * mpad + m];
  int ci[MAX_TABS];
  (void)ci;
  if constexpr (GEN) {
#pragma unroll
    for (int t = 0; t < MAX_TABS; ++t) ci[t] = t < p.n_tab ? a.test.cat[(int64_t)t * mpad + m] * p.tab_levels[t] + p.tab_off[t] : 0;
  }

  for (int idx = tid; idx < NC * SC_PIECE; idx += 256) {
    const int k = idx / SC_PIECE, j = idx - k * SC_PIECE;
    if (j < cnt) sx[j * NC + k] = a.train.xs[(int64_t)k * a.train.npad + q0 + j];
  }
  if constexpr (GEN) {
    for (int idx = tid; idx < p.n_lin * SC_PIECE; idx += 256) {
      const int k = idx / SC_PIECE, j = idx - k * SC_PIECE;
      if (j < cnt) sl[j * MAX_LIN + k] = a.train.xl[(int64_t)k * a.train.npad + q0 + j];
    }
    for (int idx = tid; idx < p.n_tab * SC_PIECE; idx += 256) {
      const int t = idx / SC_PIECE, j = idx - t * SC_PIECE;
      if (j < cnt) sc[j * MAX_TABS + t] = a.train.cat[(int64_t)t * a.train.npad + q0 + j];
    }
  }
  __syncthreads();

  auto put = [](double* o, double val, bool add) {  // (`add` is uniform: a store, or a read-modify-write of this thread's own entry)
    if (add) *o += val;
    else *o = val;
  };
  const int j_lo = wave * (SC_PIECE / 4);
  double* col = a.out + m + (q0 + j_lo) * a.ldz;
  for (int j = j_lo; j < j_lo + SC_PIECE / 4; ++j, col += a.ldz) {
    if (j >= cnt) {  // (uniform) a column of no training point
      if (!a.accumulate)
        for (int c = 0; c < a.dc; ++c) col[(int64_t)c * mpad] = 0.0;
      continue;
    }
    const double* row = sx + j * NC;
    double d[NC], r2 = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      d[k] = xi[k] - row[k];
      r2 = fma(d[k], d[k], r2);
    }
    double F = 1.0;
    if constexpr (GEN) {
#pragma unroll
      for (int t = 0; t < MAX_TABS; ++t)
        if (t < p.n_tab) F *= p.tabs[ci[t] + sc[j * MAX_TABS + t]];
    }
    const double S = real ? p.eta2 * stationary_dr2<KIND>(r2) * F : 0.0;
    if (a.periodic) {
#pragma unroll
      for (int k = 0; k + 1 < NC; k += 2)
        if (k < a.nc) {
          const double val = S * (a.scale[k >> 1] * (d[k] * xi[k + 1] - d[k + 1] * xi[k]));
          put(col + (int64_t)a.slot[k >> 1] * mpad, val, a.accumulate != 0);
        }
    } else {
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (k < a.nc) {
          const double val = S * (a.scale[k] * d[k]);
          put(col + (int64_t)a.slot[k] * mpad, val, a.accumulate != 0);
        }
    }
    if constexpr (GEN) {
      const double tf = real ? p.tau * F : 0.0;
#pragma unroll
      for (int l = 0; l < NL; ++l)
        if (l < p.n_lin) {
          const double val = tf * sl[j * MAX_LIN + l];
          put(col + (int64_t)a.slot_lin[l] * mpad, val, a.accumulate || a.lin_over[l]);
        }
    }
    if (a.zero_slots && !a.accumulate)
      for (int c = 0; c < a.dc; ++c)
        if ((a.zero_slots >> c) & 1u) col[(int64_t)c * mpad] = 0.0;
  }
}

// ---- the prior curvature P_dd per test point ----------------------------------------------------------------------------------
// prior[c * mpad + m] (+)= F_t(x*_m, x*_m) (-2 eta^2 f'(0) jj[c] + tl[c]); the test points hold term t's preparation.
struct SlopePriorArgs {
  CovParams p;
  PointSet test;
  int32_t accumulate, dc;
  double jj[SLOPE_MAX_COLS];  // J_c^2 of this term (0: no continuous share)
  double tl[SLOPE_MAX_COLS];  // tau where the column is linear in this term, else 0
  double* prior;
};

__device__ __forceinline__ double stationary_dr2_at0(int kind) {
  switch (kind) {
    case 0: return stationary_dr2<0>(0.0);
    case 1: return stationary_dr2<1>(0.0);
    default: return stationary_dr2<2>(0.0);
  }
}

__global__ __launch_bounds__(256) void slope_prior_kernel(SlopePriorArgs a) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= a.test.npad) return;
  double F = 1.0;
  for (int t = 0; t < a.p.n_tab; ++t) {
    const int c = a.test.cat[(int64_t)t * a.test.npad + m];
    F *= a.p.tabs[a.p.tab_off[t] + c * a.p.tab_levels[t] + c];
  }
  const double f0 = -2.0 * a.p.eta2 * stationary_dr2_at0(a.p.kind);
  for (int c = 0; c < a.dc; ++c) {
    const double val = F * (f0 * a.jj[c] + a.tl[c]);
    double* o = a.prior + (int64_t)c * a.test.npad + m;
    *o = a.accumulate ? *o + val : val;
  }
}

// ---- the reduction --------------------------------------------------------------------------------------------------------------
// part[chunk][q][m], q < Dc: the chunk's share of <V_q, v>; then (COV) the packed lower triangle of <V_d, V_e>, entry
// Dc + slope_tri(d, e), or (no COV) the Dc squares <V_d, V_d>, entry Dc + d.  Grid (ceil(mpad / 256), chunks, blocks): one test
// point per thread, and per instance ONE SLOPE_BLK x SLOPE_BLK block (bi, bj) of the (d, e) pairs -- 16 products + 4 dots in
// registers whatever Dc is; V is re-read per block.  The diagonal blocks also take the dots with v.  The square of column d is
// fma(x_d, x_d, .) over ascending rows with or without COV: the variance does not depend on whether the covariance was asked for.
template <bool COV>
__global__ __launch_bounds__(256) void slope_gram_partial_kernel(const double* __restrict__ V, int64_t ldz, int64_t mpad,
                                                                 const double* __restrict__ v, int64_t n, int dc,
                                                                 double* __restrict__ part) {
  constexpr int B = SLOPE_BLK;
  __shared__ double vs[RED_CHUNK];
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.y * RED_CHUNK;
  const int64_t i1 = (i0 + RED_CHUNK < n) ? i0 + RED_CHUNK : n;
  if (i0 + threadIdx.x < n) vs[threadIdx.x] = v[i0 + threadIdx.x];
  __syncthreads();
  if (m >= mpad) return;  // mpad is a multiple of 128, the block covers 256
  int bi = (int)blockIdx.z, bj = bi;
  if constexpr (COV) {
    bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= (int)blockIdx.z) ++bi;
    bj = (int)blockIdx.z - bi * (bi + 1) / 2;
  }
  const bool diag = bi == bj;
  double mu[B], g[COV ? B * B : B];
#pragma unroll
  for (int i = 0; i < B; ++i) mu[i] = 0.0;
#pragma unroll
  for (int i = 0; i < (COV ? B * B : B); ++i) g[i] = 0.0;
  // rows of the block that are no column read row 0 of the block instead (in bounds) and are never written
  int64_t offx[B], offy[B];
#pragma unroll
  for (int i = 0; i < B; ++i) {
    offx[i] = (int64_t)(B * bi + i < dc ? B * bi + i : B * bi) * mpad;
    offy[i] = (int64_t)(B * bj + i < dc ? B * bj + i : B * bj) * mpad;
  }
  const double* col = V + m + i0 * ldz;
  for (int64_t i = i0; i < i1; ++i, col += ldz) {
    double x[B], y[B];
#pragma unroll
    for (int k = 0; k < B; ++k) x[k] = col[offx[k]];
    if constexpr (COV) {
      if (diag) {
#pragma unroll
        for (int k = 0; k < B; ++k) y[k] = x[k];
      } else {
#pragma unroll
        for (int k = 0; k < B; ++k) y[k] = col[offy[k]];
      }
    }
    (void)y;
    if (diag) {
      const double vi = vs[i - i0];
#pragma unroll
      for (int k = 0; k < B; ++k) mu[k] = fma(x[k], vi, mu[k]);
    }
    if constexpr (COV) {
#pragma unroll
      for (int r = 0; r < B; ++r)
#pragma unroll
        for (int c = 0; c < B; ++c) g[r * B + c] = fma(x[r], y[c], g[r * B + c]);
    } else {
#pragma unroll
      for (int k = 0; k < B; ++k) g[k] = fma(x[k], x[k], g[k]);
    }
  }
  const int nq = slope_entries(dc, COV);
  double* out = part + (int64_t)blockIdx.y * nq * mpad + m;
#pragma unroll
  for (int r = 0; r < B; ++r) {
    const int d = B * bi + r;
    if (d >= dc) continue;
    if (diag) out[(int64_t)d * mpad] = mu[r];
    if constexpr (COV) {
#pragma unroll
      for (int c = 0; c < B; ++c) {
        const int e = B * bj + c;
        if (e <= d) out[(int64_t)(dc + slope_tri(d, e)) * mpad] = g[r * B + c];
      }
    } else {
      out[(int64_t)(dc + d) * mpad] = g[r];
    }
  }
}

// The chunks added in chunk order, one thread per test point and entry: grid (ceil(mc / 256), slope_entries).  Results go
// straight into the caller's layout (zeroed before: the other model columns stay 0): mean / var mc x D row-major, cov mc blocks of
// D x D row-major.  A covariance entry is P_de - sum, written to (d, e) AND (e, d); the diagonal entry is also the variance.
struct SlopeFinishArgs {
  const double* part;
  const double* prior;  // [Dc][mpad]
  int32_t nchunk, dc, with_cov, D;
  int64_t mpad, mc;
  int32_t col[SLOPE_MAX_COLS];  // X column of differentiable column c
  double* mean;
  double* var;
  double* cov;
};

__global__ __launch_bounds__(256) void slope_finish_kernel(SlopeFinishArgs a) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int q = (int)blockIdx.y, nq = slope_entries(a.dc, a.with_cov != 0);
  if (m >= a.mc || q >= nq) return;
  double acc = 0.0;
  for (int c = 0; c < a.nchunk; ++c) acc += a.part[((int64_t)c * nq + q) * a.mpad + m];
  if (q < a.dc) {
    a.mean[m * a.D + a.col[q]] = acc;
    return;
  }
  int d = q - a.dc, e = d;
  if (a.with_cov) {
    const int p = q - a.dc;
    d = 0;
    while ((d + 1) * (d + 2) / 2 <= p) ++d;
    e = p - d * (d + 1) / 2;
  }
  const double val = (d == e ? a.prior[(int64_t)d * a.mpad + m] : 0.0) - acc;
  if (d == e) a.var[m * a.D + a.col[d]] = val;
  if (a.with_cov) {
    double* C = a.cov + m * (int64_t)a.D * a.D;
    C[a.col[d] * a.D + a.col[e]] = val;
    C[a.col[e] * a.D + a.col[d]] = val;
  }
}

}  // namespace gmb
