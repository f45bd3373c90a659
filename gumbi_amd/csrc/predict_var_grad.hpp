// predict_var_grad.hpp -- gradient of the posterior VARIANCE with respect to the test point, d sigma^2 / d x*, in closed form and in
// one launch with the gradient of the mean (predict_grad.hpp): what a gradient-based search of an acquisition function needs
// (the reference differentiates its GPyTorch model for that purpose: gumbi/regression/botorch/GP.py, `propose`).
//
// V = K(X*, X) L^-T is what a prediction forms; with W = K(X*, X) Sigma^-1 = V L^-1 (row m = w_m)
//   sigma^2(x*)          = k(x*, x*) [+ noise] - |v|^2
//   d sigma^2 / d x*_d   = d k(x*, x*) / d x*_d - 2 sum_n W_mn d k(x*_m, x_n) / d x*_d
// The sum is predict_grad.hpp's with the weight W_mn in place of alpha_n: the same S_mn, the same accumulators A_c, the same
// finishing rules (stationary, periodic modes 1 and 2, linear, additive), the same sqrt(r^2 + 1e-12).  The prior term is 0 for
// every stationary and periodic form; a linear dimension l adds 2 tau (x*_l - c_l) F_mm, F_mm the product of the coregion table
// entries at the point's own categories.  The noise diagonal does not depend on the continuous coordinates.
//
//   vsolve_diag_kernel / vsolve_update_kernel   W <- V L^-1 in place (test index fastest): predict_grad.hpp's blocked back
//       substitution for a block of right-hand sides.  Block column b, from the last: W_b = V_b L_bb^-1 (a thread per test point,
//       the 128 x 128 solve in quarters of 32 through LDS), then V_j -= W_b L[block row b, column block j] for every j < b on
//       vector FMAs, the reduction index in ascending order.  Plain launches in stream order: no workgroup waits for another.
//       Rows and columns >= n act as identity, and W is written 0 there.
//   predict_var_grad_partial_kernel   predict_grad_partial_kernel with a second accumulator set: distance, stationary_dr2 and the
//       table product once per pair, weighted by the staged alpha_n (-> d mu) and by W[m + n mpad], a coalesced read (-> d sigma^2).
//   predict_var_grad_finish_kernel    the chunks in chunk order and the finishing rules for both sets; the variance set times -2,
//       plus the prior term.
// No atomics, fixed summation orders: the same bits call after call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covariance.hpp"
#include "gradient.hpp"
#include "predict_grad.hpp"

namespace gmb {

// ---- W <- V L^-1 ---------------------------------------------------------------------------------------------------------------
constexpr int VS_ROWS = 128;  // test points per workgroup of the diagonal solve (a thread each)
constexpr int VS_PTS = 64;    // test points per workgroup of the update (a lane each; four waves split the 128 columns)
constexpr int VS_KSTEP = 32;  // rows of L staged at a time by the update
constexpr int VS_LDT = 130;   // row stride of the staged rows (even: 16-byte aligned rows)
constexpr int VS_LDQ = 32;    // ... and of the diagonal solve's 32 x 32 tiles

// W_b = V_b L_bb^-1 for the 128 columns of block b, every row of the M-tile, in quarters of 32 columns from the last: quarter q
// takes v_q - sum_{p > q} x_p L_pq (x_p: this thread's own earlier stores) and solves against L_qq.  Thread m keeps the quarter's
// 32 unknowns in registers; the 32 x 32 tiles of L go through LDS, every read of them a broadcast.  The grid covers mpad / 128.
__global__ __launch_bounds__(VS_ROWS) void vsolve_diag_kernel(TriOperand L, int64_t b, int64_t n, double* V, int64_t mpad) {
  __shared__ double T[32 * VS_LDQ];
  const int tid = threadIdx.x;
  const int64_t m = (int64_t)blockIdx.x * VS_ROWS + tid;
  const int64_t base = b * 128;
  auto stage = [&](int r0, int c0) {  // T[k * VS_LDQ + j] = L(base + r0 + k, base + c0 + j), identity beyond n
    __syncthreads();
    for (int idx = tid; idx < 32 * 32; idx += VS_ROWS) {
      const int j = idx >> 5, k = idx & 31;  // k fastest: contiguous in the column-major tile
      const int64_t gi = base + r0 + k, gj = base + c0 + j;
      double v = gi == gj ? 1.0 : 0.0;
      if (gi < n && gj < n && gj <= gi) v = tri_at(L, gi, gj);
      T[k * VS_LDQ + j] = v;
    }
    __syncthreads();
  };
  for (int q = 3; q >= 0; --q) {
    double* vq = V + m + (base + 32 * q) * mpad;
    double x[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) x[j] = base + 32 * q + j < n ? vq[(int64_t)j * mpad] : 0.0;
    for (int p = 3; p > q; --p) {  // (a fixed order: quarters from the last, rows ascending)
      stage(32 * p, 32 * q);
      const double* xp = V + m + (base + 32 * p) * mpad;
      for (int k = 0; k < 32; ++k) {
        const double xk = xp[(int64_t)k * mpad];
#pragma unroll
        for (int j = 0; j < 32; ++j) x[j] = fma(-xk, T[k * VS_LDQ + j], x[j]);
      }
    }
    stage(32 * q, 32 * q);
#pragma unroll
    for (int k = 31; k >= 0; --k) {  // unknowns from the last
      const double xk = x[k] / T[k * VS_LDQ + k];
      x[k] = xk;
#pragma unroll
      for (int j = 0; j < 32; ++j)
        if (j < k) x[j] = fma(-xk, T[k * VS_LDQ + j], x[j]);
    }
#pragma unroll
    for (int j = 0; j < 32; ++j) vq[(int64_t)j * mpad] = x[j];
  }
}

// V_j -= W_b L[block row b, column block j]: grid (mpad / 64, b); lane = test point, wave w owns columns 32 w .. 32 w + 31 of
// column block j = blockIdx.y.  The rows i of block b are staged 32 at a time and added in ascending order.
__global__ __launch_bounds__(256) void vsolve_update_kernel(TriOperand L, int64_t b, int64_t n, double* V, int64_t mpad) {
  __shared__ double T[VS_KSTEP * VS_LDT];  // T[i * VS_LDT + c] = L(base + q + i, 128 j + c)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m = (int64_t)blockIdx.x * VS_PTS + lane;
  const int64_t base = b * 128, cb = (int64_t)blockIdx.y * 128;
  double acc[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) acc[c] = 0.0;
  for (int q = 0; q < 128; q += VS_KSTEP) {
    __syncthreads();
    for (int idx = tid; idx < VS_KSTEP * 128; idx += 256) {
      const int i = idx & (VS_KSTEP - 1), c = idx / VS_KSTEP;  // i fastest: contiguous down a column of L
      const int64_t gi = base + q + i;
      // (column cb + c < 128 b <= n lies in an earlier block column than row gi: the off-diagonal part of the operand)
      T[i * VS_LDT + c] = gi < n ? L.A[gi + (cb + c) * L.ld] : 0.0;
    }
    __syncthreads();
    for (int i = 0; i < VS_KSTEP; ++i) {
      const int64_t gi = base + q + i;
      const double w = gi < n ? V[m + gi * mpad] : 0.0;
      const double* row = T + i * VS_LDT + wave * 32;
#pragma unroll
      for (int c = 0; c < 32; ++c) acc[c] = fma(w, row[c], acc[c]);
    }
  }
  double* out = V + m + (cb + wave * 32) * mpad;
#pragma unroll
  for (int c = 0; c < 32; ++c) out[(int64_t)c * mpad] -= acc[c];
}

// ---- the fused gradient kernel -----------------------------------------------------------------------------------------------
// Workgroup shape, staging and chunking are predict_grad_partial_kernel's (PG_PTS, PG_PIECE, predict_grad_chunk).  Partials:
// [chunk][set][accumulator][mpad], set 0 weighted by alpha (d mu), set 1 by W (d sigma^2); accumulators as in PredGradArgs.
struct PredVarGradArgs {
  CovParams p;
  PointSet test;        // mpad a multiple of 128
  PointSet train;
  const double* alpha;  // Sigma^-1 y, length >= train.n
  const double* W;      // K(X*, X) Sigma^-1: W[m + n * test.npad]
  double* part;
  int64_t chunk;
};

template <int KIND, int NC, bool GEN>
__global__ __launch_bounds__(256) void predict_var_grad_partial_kernel(PredVarGradArgs a) {
  constexpr int NCS = (NC + 2) & ~1;
  constexpr int NL = GEN ? MAX_LIN : 0;
  constexpr int NACC = NC + NL;
  constexpr int STAGE = PG_PIECE * NCS + PG_PIECE * NL + (GEN ? PG_PIECE * MAX_TABS / 2 : 0);  // doubles
  constexpr int RED = 3 * NACC * PG_PTS;  // one set at a time
  __shared__ double smem[STAGE > RED ? STAGE : RED];
  double* sx = smem;                                                    // [PG_PIECE][NCS]
  double* sl = smem + PG_PIECE * NCS;                                   // [PG_PIECE][MAX_LIN]
  int32_t* sc = reinterpret_cast<int32_t*>(smem + PG_PIECE * (NCS + NL));  // [PG_PIECE][MAX_TABS]
  (void)sl;
  (void)sc;
  const CovParams& p = a.p;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m = (int64_t)blockIdx.x * PG_PTS + lane;  // < test.npad
  const int64_t n0 = (int64_t)blockIdx.y * a.chunk;
  const int64_t n1 = n0 + a.chunk < a.train.n ? n0 + a.chunk : a.train.n;

  double xi[NC], acc[2][NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    xi[k] = a.test.xs[(int64_t)k * a.test.npad + m];
    acc[0][k] = acc[1][k] = 0.0;
  }
  double lin[2][NL > 0 ? NL : 1];
  int ci[MAX_TABS];
  (void)lin;
  (void)ci;
  if constexpr (GEN) {
#pragma unroll
    for (int l = 0; l < NL; ++l) lin[0][l] = lin[1][l] = 0.0;
#pragma unroll
    for (int t = 0; t < MAX_TABS; ++t) ci[t] = t < p.n_tab ? a.test.cat[(int64_t)t * a.test.npad + m] * p.tab_levels[t] + p.tab_off[t] : 0;
  }

  for (int64_t q0 = n0; q0 < n1; q0 += PG_PIECE) {
    const int cnt = (int)(n1 - q0 < PG_PIECE ? n1 - q0 : PG_PIECE);
    __syncthreads();  // the previous piece has been read
    for (int idx = tid; idx < (NC + 1) * PG_PIECE; idx += 256) {
      const int k = idx / PG_PIECE, j = idx - k * PG_PIECE;
      if (j < cnt) sx[j * NCS + k] = k < NC ? a.train.xs[(int64_t)k * a.train.npad + q0 + j] : a.alpha[q0 + j];
    }
    if constexpr (GEN) {
      for (int idx = tid; idx < p.n_lin * PG_PIECE; idx += 256) {
        const int k = idx / PG_PIECE, j = idx - k * PG_PIECE;
        if (j < cnt) sl[j * MAX_LIN + k] = a.train.xl[(int64_t)k * a.train.npad + q0 + j];
      }
      for (int idx = tid; idx < p.n_tab * PG_PIECE; idx += 256) {
        const int t = idx / PG_PIECE, j = idx - t * PG_PIECE;
        if (j < cnt) sc[j * MAX_TABS + t] = a.train.cat[(int64_t)t * a.train.npad + q0 + j];
      }
    }
    __syncthreads();
    const int j_lo = wave * (PG_PIECE / 4);
    const int j_hi = j_lo + PG_PIECE / 4 < cnt ? j_lo + PG_PIECE / 4 : cnt;
    const double* wcol = a.W + m + (q0 + j_lo) * a.test.npad;  // q0 + j < n1 <= train.n for every j read below
#pragma unroll 2
    for (int j = j_lo; j < j_hi; ++j, wcol += a.test.npad) {
      const double* row = sx + j * NCS;
      double d[NC], r2 = 0.0;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        d[k] = xi[k] - row[k];
        r2 = fma(d[k], d[k], r2);
      }
      double fa = row[NC];  // alpha_n (times F_mn)
      double fw = *wcol;    // W_mn (times F_mn)
      if constexpr (GEN) {
        double F = 1.0;
#pragma unroll
        for (int t = 0; t < MAX_TABS; ++t)
          if (t < p.n_tab) F *= p.tabs[ci[t] + sc[j * MAX_TABS + t]];
        fa *= F;
        fw *= F;
#pragma unroll
        for (int l = 0; l < NL; ++l)
          if (l < p.n_lin) {
            const double xl = sl[j * MAX_LIN + l];
            lin[0][l] = fma(fa, xl, lin[0][l]);
            lin[1][l] = fma(fw, xl, lin[1][l]);
          }
      }
      const double g = p.eta2 * stationary_dr2<KIND>(r2);
      const double s0 = g * fa, s1 = g * fw;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        acc[0][k] = fma(s0, d[k], acc[0][k]);
        acc[1][k] = fma(s1, d[k], acc[1][k]);
      }
    }
  }

  // per set: waves 1 .. 3 hand their accumulators to wave 0, which adds them in wave order and writes the chunk's partials
  const int nacc = NC + p.n_lin;
  double* red = smem;  // [3][NACC][PG_PTS]
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    __syncthreads();  // the staging area (or the previous set) is free
    if (wave > 0) {
#pragma unroll
      for (int k = 0; k < NC; ++k) red[((wave - 1) * NACC + k) * PG_PTS + lane] = acc[s][k];
      if constexpr (GEN) {
#pragma unroll
        for (int l = 0; l < NL; ++l) red[((wave - 1) * NACC + NC + l) * PG_PTS + lane] = lin[s][l];
      }
    }
    __syncthreads();
    if (wave == 0) {
      double* out = a.part + ((int64_t)blockIdx.y * 2 + s) * nacc * a.test.npad + m;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        double v = acc[s][k];
#pragma unroll
        for (int w = 0; w < 3; ++w) v += red[(w * NACC + k) * PG_PTS + lane];
        out[(int64_t)k * a.test.npad] = v;
      }
      if constexpr (GEN) {
#pragma unroll
        for (int l = 0; l < NL; ++l)
          if (l < p.n_lin) {
            double v = lin[s][l];
#pragma unroll
            for (int w = 0; w < 3; ++w) v += red[(w * NACC + NC + l) * PG_PTS + lane];
            out[(int64_t)(NC + l) * a.test.npad] = v;
          }
      }
    }
  }
}

// Sum of the chunks in chunk order, then predict_grad_finish_kernel's rules for both sets; ADDS the term's gradients to dmean and
// dvar (mc x D row-major, zeroed by the caller before the first term).  One thread per test point.
struct PredVarGradFinishArgs {
  PredGradFinishArgs f;  // part, nchunk, ..., grad = d mu
  double* dvar;
  CovParams p;           // the term's tables (prior term of the linear dimensions)
  const double* txl;     // prepared test points: linear coordinates minus c, categories
  const int32_t* tcat;
};

__global__ __launch_bounds__(256) void predict_var_grad_finish_kernel(PredVarGradFinishArgs a) {
  const PredGradFinishArgs& f = a.f;
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= f.mc) return;
  const int nacc = f.nc_pad + f.n_lin;
  for (int s = 0; s < 2; ++s) {
    auto total = [&](int acc) {
      double t = 0.0;
      for (int c = 0; c < f.nchunk; ++c) t += f.part[(((int64_t)c * 2 + s) * nacc + acc) * f.mpad + m];
      return t;
    };
    double* g = (s ? a.dvar : f.grad) + m * f.D;
    const double sign = s ? -2.0 : 1.0;
    if (f.periodic) {
      for (int d = 0; 2 * d < f.nc; ++d) {
        const double us = f.txs[(int64_t)(2 * d) * f.mpad + m], uc = f.txs[(int64_t)(2 * d + 1) * f.mpad + m];
        g[f.idx_cont[2 * d]] += sign * (f.scale[d] * (total(2 * d) * uc - total(2 * d + 1) * us));
      }
    } else {
      for (int k = 0; k < f.nc; ++k) g[f.idx_cont[k]] += sign * (f.scale[k] * total(k));
    }
    for (int l = 0; l < f.n_lin; ++l) g[f.idx_lin[l]] += sign * (f.tau * total(f.nc_pad + l));
  }
  if (f.n_lin > 0) {  // d k(x*, x*) / d x*_l = 2 tau (x*_l - c_l) F_mm
    double F = 1.0;
    for (int t = 0; t < a.p.n_tab; ++t) {
      const int c = a.tcat[(int64_t)t * f.mpad + m];
      F *= a.p.tabs[a.p.tab_off[t] + c * a.p.tab_levels[t] + c];
    }
    double* g = a.dvar + m * f.D;
    for (int l = 0; l < f.n_lin; ++l) g[f.idx_lin[l]] += 2.0 * f.tau * a.txl[(int64_t)l * f.mpad + m] * F;
  }
}

}  // namespace gmb
