// predict_grad.hpp -- gradients of the posterior mean and variance with respect to the test point, d mu / d x* and
// d sigma^2 / d x*, in closed form (the reference differentiates its GPyTorch model by autograd:
// gumbi/regression/botorch/GP.py:535-576, and `propose` for the search of an acquisition function).
//
// One term of the model is  k(x*, x) = [eta^2 f(r^2) + tau sum_l (x*_l - c_l)(x_l - c_l)] F(x*, x),  F the product of the
// coregion table entries (no continuous coordinate in it).  With mu(x*) = sum_n k(x*, x_n) alpha_n, alpha = Sigma^-1 y,
//   d mu / d x*_d = sum_n alpha_n F_mn [ eta^2 f'(r^2_mn) d r^2_mn / d x*_d + tau (x_nd - c_d) 1{d linear} ],  f' = stationary_dr2
// (which keeps sqrt(r^2 + 1e-12): Matern-1/2 and Exponential are smooth, their gradient at a coincident point is 0).
// On the prepared columns u = x / ls, with  S_mn = eta^2 f'(r^2_mn) F_mn alpha_n  and  A_c = sum_n S_mn (u*_mc - u_nc):
//   stationary         G_d = 2 inv_ls_d A_d
//   periodic (1, 2)    columns (2d, 2d + 1) = w_d (sin t, cos t), t = 2 pi x / T_d:
//                      G_d = 2 (2 pi / T_d) (A_2d u*_(2d+1) - A_(2d+1) u*_2d)      (mode 2's w = 1 / (2 ls) rides in the columns)
//   linear             G_l += tau sum_n F_mn alpha_n xl_nl
// Additive models sum their terms; categorical / output columns get 0.
//
// The variance.  V = K(X*, X) L^-T is what a prediction forms; with W = K(X*, X) Sigma^-1 = V L^-1 (row m = w_m)
//   sigma^2(x*)          = k(x*, x*) [+ noise] - |v|^2
//   d sigma^2 / d x*_d   = d k(x*, x*) / d x*_d - 2 sum_n W_mn d k(x*_m, x_n) / d x*_d
// The sum is the mean's with the weight W_mn in place of alpha_n: the same S_mn, the same accumulators A_c, the same finishing
// rules, the same sqrt(r^2 + 1e-12).  The prior term is 0 for every stationary and periodic form; a linear dimension l adds
// 2 tau (x*_l - c_l) F_mm, F_mm the product of the coregion table entries at the point's own categories.  The noise diagonal
// does not depend on the continuous coordinates.
//
// predict_grad_partial_kernel<KIND, NC, GEN, NSET> forms the A_c (and the linear sums) of one block of test points against one
// CHUNK of training points from direct scaled differences -- the expansion sum S u* - sum S u_n cancels where the gradient is
// small.  NSET = 1: the set weighted by alpha (d mu).  NSET = 2: a second accumulator set weighted by W[m + n mpad], a coalesced
// read (d sigma^2); distance, stationary_dr2 and the table entries once per pair.  Set 0's arithmetic is the same operations
// in both, so d mu / d x* does not depend on which was launched.  predict_grad_finish_kernel adds the chunks in fixed order and
// applies the rules above; the variance set times -2, plus the prior term.  No atomics: the same bits call after call.  Nothing
// of size M x N is written: O(M N d) arithmetic, partials of (chunks x sets x accumulators x M) doubles.
//
// alpha itself: a gradient evaluation leaves it resident; behind a bare factorisation it comes from a blocked back substitution
// L^T alpha = v (backsub_* below): plain launches in stream order, one 128 x 128 transposed solve + one block-row update per
// block column.  W <- V L^-1 in place (test index fastest) is the same substitution for a block of right-hand sides
// (vsolve_* below).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covariance.hpp"
#include "gradient.hpp"

namespace gmb {

// ---- the fused gradient kernel -----------------------------------------------------------------------------------------------
// A workgroup = 64 test points (one per lane) x 4 waves; the waves split every staged piece of the workgroup's training chunk
// four ways, so each LDS read is a broadcast and a block of 64 test points already gives four waves of work.  The four
// waves' accumulators are added in the fixed order 0 + 1 + 2 + 3 through LDS at the end.
constexpr int PG_PTS = 64;      // test points per workgroup
constexpr int PG_PIECE = 128;   // training points staged in LDS at a time
constexpr int PG_UNIT = 64;     // chunk lengths are multiples of this
// Chunk length (predict_grad_chunk): as long as possible -- every chunk costs one set of partials, (NC + n_lin) x mpad doubles,
// and one more pass of the finishing sum -- while the grid keeps PG_TARGET_WGS workgroups, two waves per SIMD of the 256
// compute units.  M = 10^4 behind N = 10^4: 157 point blocks -> 7 chunks of 1472 (partials = 7 x the output's continuous
// part); M = 128 behind N = 10^4: 2 point blocks -> the floor of 64 training points per chunk, 314 workgroups on 256 compute
// units (partials: 157 x 128 x d doubles, 0.6 MB at d = 4).  Either way the partials hold at most
// (PG_TARGET_WGS x 64 + mpad) x (NC + n_lin) doubles: a small multiple of M d for large M, 13 MB at worst for small M.
constexpr int PG_TARGET_WGS = 1024;

inline void predict_grad_chunk(int64_t N, int64_t mpad, int64_t* chunk, int* nchunk) {
  const int64_t mblocks = mpad / PG_PTS;
  int64_t want = (PG_TARGET_WGS + mblocks - 1) / mblocks;
  const int64_t most = (N + PG_UNIT - 1) / PG_UNIT;
  want = want < 1 ? 1 : (want > most ? most : want);
  int64_t len = (N + want - 1) / want;
  len = (len + PG_UNIT - 1) / PG_UNIT * PG_UNIT;
  *chunk = len;
  *nchunk = (int)((N + len - 1) / len);
}

struct PredGradArgs {
  CovParams p;
  PointSet test;        // mpad a multiple of 128
  PointSet train;
  const double* alpha;  // Sigma^-1 y, length >= train.n
  double* part;         // [chunk][set][accumulator][mpad]: accumulators 0 .. NC-1 = A_c, NC .. NC + n_lin - 1 = the linear sums;
                        // set 0 weighted by alpha (d mu), set 1 (NSET == 2 only) by W (d sigma^2)
  int64_t chunk;        // training points per chunk (a multiple of PG_UNIT)
  const double* W;      // K(X*, X) Sigma^-1: W[m + n * test.npad]; read only when NSET == 2
};

template <int KIND, int NC, bool GEN, int NSET>
__global__ __launch_bounds__(256) void predict_grad_partial_kernel(PredGradArgs a) {
  constexpr int NCS = (NC + 2) & ~1;             // row stride of the staged points: NC coordinates, alpha, padded to even
  constexpr int NL = GEN ? MAX_LIN : 0;
  constexpr int NACC = NC + NL;
  constexpr int STAGE = PG_PIECE * NCS + PG_PIECE * NL + (GEN ? PG_PIECE * MAX_TABS / 2 : 0);  // doubles
  constexpr int RED = 3 * NACC * PG_PTS;         // one set at a time
  __shared__ double smem[STAGE > RED ? STAGE : RED];
  double* sx = smem;                                                    // [PG_PIECE][NCS]
  double* sl = smem + PG_PIECE * NCS;                                   // [PG_PIECE][MAX_LIN]
  int32_t* sc = reinterpret_cast<int32_t*>(smem + PG_PIECE * (NCS + NL));  // [PG_PIECE][MAX_TABS]
  (void)sl;
  (void)sc;
  const CovParams& p = a.p;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m = (int64_t)blockIdx.x * PG_PTS + lane;  // < test.npad: the grid covers mpad / 64 blocks exactly
  const int64_t n0 = (int64_t)blockIdx.y * a.chunk;
  const int64_t n1 = n0 + a.chunk < a.train.n ? n0 + a.chunk : a.train.n;  // training rows >= N contribute nothing

  double xi[NC], acc[NSET][NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    xi[k] = a.test.xs[(int64_t)k * a.test.npad + m];
#pragma unroll
    for (int s = 0; s < NSET; ++s) acc[s][k] = 0.0;
  }
  double lin[NSET][NL > 0 ? NL : 1];
  int ci[MAX_TABS];
  (void)lin;
  (void)ci;
  if constexpr (GEN) {
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
      for (int s = 0; s < NSET; ++s) lin[s][l] = 0.0;
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
    const double* wcol = nullptr;  // q0 + j < n1 <= train.n for every j read below
    (void)wcol;
    if constexpr (NSET == 2) wcol = a.W + m + (q0 + j_lo) * a.test.npad;
#pragma unroll 2
    for (int j = j_lo; j < j_hi; ++j) {
      const double* row = sx + j * NCS;
      double d[NC], r2 = 0.0;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        d[k] = xi[k] - row[k];
        r2 = fma(d[k], d[k], r2);
      }
      double fa[NSET];  // alpha_n, W_mn (times F_mn)
      fa[0] = row[NC];
      if constexpr (NSET == 2) {
        fa[1] = *wcol;
        wcol += a.test.npad;
      }
      if constexpr (GEN) {
#pragma unroll
        for (int t = 0; t < MAX_TABS; ++t)
          if (t < p.n_tab) {
            const double b = p.tabs[ci[t] + sc[j * MAX_TABS + t]];
#pragma unroll
            for (int s = 0; s < NSET; ++s) fa[s] *= b;
          }
#pragma unroll
        for (int l = 0; l < NL; ++l)
          if (l < p.n_lin) {
            const double xl = sl[j * MAX_LIN + l];
#pragma unroll
            for (int s = 0; s < NSET; ++s) lin[s][l] = fma(fa[s], xl, lin[s][l]);
          }
      }
      const double g = p.eta2 * stationary_dr2<KIND>(r2);
#pragma unroll
      for (int s = 0; s < NSET; ++s) {
        const double w = g * fa[s];
#pragma unroll
        for (int k = 0; k < NC; ++k) acc[s][k] = fma(w, d[k], acc[s][k]);
      }
    }
  }

  // per set: waves 1 .. 3 hand their accumulators to wave 0, which adds them in wave order and writes the chunk's partials
  const int nacc = NC + p.n_lin;
  double* red = smem;  // [3][NACC][PG_PTS]
#pragma unroll
  for (int s = 0; s < NSET; ++s) {
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
      double* out = a.part + ((int64_t)blockIdx.y * NSET + s) * nacc * a.test.npad + m;
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

// Sum of the chunks in chunk order, then the finishing rules, per set; ADDS the term's gradient to grad (set 0) and, times -2
// and with the prior term, to dvar (set 1, nset == 2 only): mc x D row-major, zeroed by the caller before the first term.  One
// thread per test point.
struct PredGradFinishArgs {
  const double* part;
  int32_t nchunk, nc, nc_pad, n_lin, periodic, D, nset;
  int64_t mpad, mc;
  const double* txs;        // prepared test coordinates (periodic rule)
  int32_t idx_cont[16];     // X column per prepared column
  double scale[16];         // stationary: 2 inv_ls per prepared column; periodic: 2 (2 pi / T_d) per DIMENSION d
  int32_t idx_lin[MAX_LIN];
  double tau;
  double* grad;
  // nset == 2 only: the variance gradient, and for its prior term the term's tables and the prepared test points' linear
  // coordinates (minus c) and categories
  double* dvar;
  int32_t n_tab, tab_levels[MAX_TABS], tab_off[MAX_TABS];
  const double* tabs;
  const double* txl;
  const int32_t* tcat;
};

template <int SET>
__device__ __forceinline__ void predict_grad_finish_set(const PredGradFinishArgs& a, int64_t m) {
  const int nacc = a.nc_pad + a.n_lin;
  auto total = [&](int acc) {
    double s = 0.0;
    for (int c = 0; c < a.nchunk; ++c) s += a.part[(((int64_t)c * a.nset + SET) * nacc + acc) * a.mpad + m];
    return s;
  };
  double* g = (SET ? a.dvar : a.grad) + m * a.D;
  auto add = [&](int col, double v) {
    if constexpr (SET == 0) g[col] += v;
    else g[col] += -2.0 * v;
  };
  if (a.periodic) {
    for (int d = 0; 2 * d < a.nc; ++d) {
      const double us = a.txs[(int64_t)(2 * d) * a.mpad + m], uc = a.txs[(int64_t)(2 * d + 1) * a.mpad + m];
      add(a.idx_cont[2 * d], a.scale[d] * (total(2 * d) * uc - total(2 * d + 1) * us));
    }
  } else {
    for (int k = 0; k < a.nc; ++k) add(a.idx_cont[k], a.scale[k] * total(k));
  }
  for (int l = 0; l < a.n_lin; ++l) add(a.idx_lin[l], a.tau * total(a.nc_pad + l));
}

__global__ __launch_bounds__(256) void predict_grad_finish_kernel(PredGradFinishArgs a) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= a.mc) return;
  predict_grad_finish_set<0>(a, m);
  if (a.nset < 2) return;
  predict_grad_finish_set<1>(a, m);
  if (a.n_lin > 0) {  // d k(x*, x*) / d x*_l = 2 tau (x*_l - c_l) F_mm
    double F = 1.0;
    for (int t = 0; t < a.n_tab; ++t) {
      const int c = a.tcat[(int64_t)t * a.mpad + m];
      F *= a.tabs[a.tab_off[t] + c * a.tab_levels[t] + c];
    }
    double* g = a.dvar + m * a.D;
    for (int l = 0; l < a.n_lin; ++l) g[a.idx_lin[l]] += 2.0 * a.tau * a.txl[(int64_t)l * a.mpad + m] * F;
  }
}

// ---- alpha = L^-T v by blocked back substitution ------------------------------------------------------------------------------
// L is read through a TriOperand (diagonal tiles possibly apart from the rest), rows and columns >= n act as identity (row n of
// the factor buffer is the y row, not part of L).  w starts as v; block column b, from the last:
//   backsub_diag_kernel    alpha_b = L_bb^-T w_b                      one workgroup
//   backsub_update_kernel  w_j -= sum_{i in block b} L(i, j) alpha_i  for every column j < 128 b, one wave per column
// in stream order -- no workgroup waits for another.

// The 128 x 128 transposed solve in two halves of 64 through one 64 x 65 LDS buffer: x_hi from L22, w_lo -= L21^T x_hi, x_lo
// from L11.  All 256 threads stage; the first wave solves (lane j owns unknown j: no barrier inside a half).
__global__ __launch_bounds__(256) void backsub_diag_kernel(TriOperand L, int64_t b, int64_t n, const double* __restrict__ w,
                                                           double* __restrict__ alpha) {
  __shared__ double T[64 * 65];
  __shared__ double xh[64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t base = b * 128;
  auto stage = [&](int r0, int c0) {  // T[k * 65 + j] = L(base + r0 + k, base + c0 + j), identity beyond n
    __syncthreads();
    for (int idx = tid; idx < 64 * 64; idx += 256) {
      const int j = idx >> 6, k = idx & 63;  // k fastest: contiguous in the column-major tile
      const int64_t gi = base + r0 + k, gj = base + c0 + j;
      double v = gi == gj ? 1.0 : 0.0;
      if (gi < n && gj < n && gj <= gi) v = tri_at(L, gi, gj);
      T[k * 65 + j] = v;
    }
    __syncthreads();
  };
  auto solve = [&](double rhs) {  // first wave: unknowns from the last; returns x_lane
    double x = 0.0;
    for (int k = 63; k >= 0; --k) {
      const double xk = __shfl(rhs, k) / T[k * 65 + k];
      if (lane == k) x = xk;
      if (lane < k) rhs = fma(-T[k * 65 + lane], xk, rhs);
    }
    return x;
  };
  double w_lo = 0.0;
  stage(64, 64);
  if (tid < 64) {
    const int64_t gi = base + 64 + lane;
    const double x = solve(gi < n ? w[gi] : 0.0);
    xh[lane] = x;
    alpha[gi] = x;
  }
  stage(64, 0);  // (its barriers also publish xh)
  if (tid < 64) {
    w_lo = base + lane < n ? w[base + lane] : 0.0;
    for (int k = 0; k < 64; ++k) w_lo = fma(-T[k * 65 + lane], xh[k], w_lo);
  }
  stage(0, 0);
  if (tid < 64) alpha[base + lane] = solve(w_lo);
}

__global__ __launch_bounds__(256) void backsub_update_kernel(TriOperand L, int64_t b, int64_t n, const double* __restrict__ alpha,
                                                             double* __restrict__ w) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + wave;  // < 128 b: the grid covers the columns exactly
  const int64_t i0 = b * 128 + lane, i1 = i0 + 64;
  // (j is in an earlier block column than rows i0, i1: the off-diagonal part of the operand)
  double s = i0 < n ? L.A[i0 + j * L.ld] * alpha[i0] : 0.0;
  if (i1 < n) s = fma(L.A[i1 + j * L.ld], alpha[i1], s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
  if (lane == 0) w[j] -= s;
}

// ---- W <- V L^-1 in place (test index fastest): the same substitution for a block of right-hand sides ---------------------------
// Block column b, from the last: W_b = V_b L_bb^-1 (vsolve_diag_kernel: a thread per test point, the 128 x 128 solve in quarters
// of 32 through LDS), then V_j -= W_b L[block row b, column block j] for every j < b (vsolve_update_kernel: vector FMAs, the
// reduction index in ascending order).  Plain launches in stream order: no workgroup waits for another.  Rows and columns >= n
// act as identity, and W is written 0 there.
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

}  // namespace gmb
