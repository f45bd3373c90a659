// fitc.hpp -- the kernels of the sparse (FITC) path that are its own.  PyMC's MarginalSparse(approx="FITC") on m
// inducing points Z, restated:
//
//   Kuu = k(Z, Z) + jitter I = Lu Lu^T      A = Lu^-1 k(Z, X)  (m x N)      lambda_i = max(k_ii - sum_k A_ki^2, 0) + sigma^2
//   B = I + A Lambda^-1 A^T = L_B L_B^T     c = L_B^-1 A Lambda^-1 y       w = L_B^-T c
//   NLML = 1/2 sum log lambda + sum log diag L_B + 1/2 (y^T Lambda^-1 y - c^T c) + N/2 log 2 pi
//
// X is walked in column tiles (fitc_plan.hpp).  A tile's block lives in two layouts: "V" with the tile's column index fastest
// (V[n + k * tpad] = A[k, n]: what the cross-covariance launch writes and the engine's triangular solves work on, the inducing
// points in the role of the training set) and "S" with the inducing index fastest (S[k + n * mr]: the operand layout of the f64
// GEMM, whose contraction index is the slow one).  The cross-covariance, the solves, the GEMM, the Cholesky and the transposes are
// the engine's; here are
//   fitc_column_kernel   lambda and the NLML's column sums of a tile, and the scaled block A Lambda^-1/2 in the S layout with
//                        y Lambda^-1/2 as its border row m -- so that ONE product S S^T adds the tile's share of B, of
//                        u = A Lambda^-1 y (row m of the bordered matrix: the factorisation turns it into c) and of y^T Lambda^-1 y
//   fitc_row_kernel      the gradient's alpha, d and the scaling C Lambda^-1 of a tile
//   fitc_adjoint_kernel  T = H - w alpha^T - A diag(d), one elementwise pass
//   fitc_deriv_kernel    sum G o dk(P, Q)/dtheta_j for every theta_j of the kernel at once over a rectangular block, the kernel
//                        derivative formed from the prepared coordinates in registers; nothing of size m x N x P is written
//   fitc_fold_kernel     the fixed-order second stage of every sum above
//   fitc_predict_kernel  mean = As^T w and var = k** - colsum(As^2) + colsum(C*^2) in one pass
// Every sum has a fixed order (no atomics): the same bits call after call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covariance.hpp"
#include "fitc_plan.hpp"

namespace gmb {

// ---- pass 1: a tile's columns --------------------------------------------------------------------------------------------------
struct FitcColArgs {
  const double* At;  // At[n + k * ldt] = A[k, first + n]
  int64_t ldt;       // = tpad
  int64_t tc;        // real columns of the tile
  int32_t m;
  int64_t mr;
  const double* y;   // of the tile's first column on (as lam and part are)
  double kdiag;      // k(x, x) of the stationary kernel: eta^2
  double sigma2;
  double* lam;
  double* S;         // S[k + n * mr], mr rows x tpad columns, every element written
  double* part;      // [block of 32 columns][FITC_COL_SUMS]: slots 0 (sum log lambda) and 1 (sum y^2 / lambda)
};

// A workgroup owns FITC_COL_BLOCK = 32 columns: thread (tx, ty) = (tid & 31, tid >> 5) adds the rows k = ty, ty + 8, ... of column
// tx, the eight partial sums are added in ascending ty.  The scaled block then goes through a 32 x 33 LDS tile, so that both the
// reads of At and the writes of S run along their fast index.
__global__ __launch_bounds__(256) void fitc_column_kernel(FitcColArgs a) {
  __shared__ double qp[8][32];
  __shared__ double rs[32], ys[32], t0[32], t1[32];
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t n0 = (int64_t)blockIdx.x * FITC_COL_BLOCK;
  const int64_t n = n0 + tx;
  const bool real = n < a.tc;
  double q = 0.0;
  if (real)
    for (int k = ty; k < a.m; k += 8) {
      const double v = a.At[n + (int64_t)k * a.ldt];
      q = fma(v, v, q);
    }
  qp[ty][tx] = q;
  __syncthreads();
  if (ty == 0) {
    double r = 0.0, yr = 0.0, l0 = 0.0, l1 = 0.0;
    if (real) {
      double s = qp[0][tx];
#pragma unroll
      for (int j = 1; j < 8; ++j) s += qp[j][tx];
      const double lam = fmax(a.kdiag - s, 0.0) + a.sigma2;  // (the clip as PyMC applies it: a constant for the gradient)
      a.lam[n] = lam;
      r = 1.0 / sqrt(lam);
      yr = a.y[n] * r;
      l0 = log(lam);
      l1 = yr * yr;
    }
    rs[tx] = r;
    ys[tx] = yr;
    t0[tx] = l0;
    t1[tx] = l1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s0 = 0.0, s1 = 0.0;
    for (int j = 0; j < 32; ++j) s0 += t0[j], s1 += t1[j];
    a.part[(int64_t)blockIdx.x * FITC_COL_SUMS + 0] = s0;
    a.part[(int64_t)blockIdx.x * FITC_COL_SUMS + 1] = s1;
  }
  for (int64_t k0 = 0; k0 < a.mr; k0 += 32) {
    for (int j = ty; j < 32; j += 8) {
      const int64_t k = k0 + j;
      double v = 0.0;
      if (real) v = k < a.m ? a.At[n + k * a.ldt] * rs[tx] : (k == a.m ? ys[tx] : 0.0);
      tile[j][tx] = v;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) a.S[(k0 + tx) + (n0 + j) * a.mr] = tile[tx][j];
    __syncthreads();
  }
}

// out[q] (+)= sum_b part[b * stride + q], q < nvals: ONE workgroup; thread t adds the blocks t, t + 256, ... in ascending order,
// then a fixed LDS tree.  Launches follow each other in stream order, so an accumulating fold adds the tiles in a fixed order too.
__global__ __launch_bounds__(256) void fitc_fold_kernel(const double* __restrict__ part, int64_t nblocks, int stride, int q0, int nvals,
                                                        double* out, int accumulate) {
  __shared__ double red[256];
  for (int q = 0; q < nvals; ++q) {
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < nblocks; b += 256) s += part[b * stride + q0 + q];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[q] = accumulate ? out[q] + red[0] : red[0];
    __syncthreads();
  }
}

// B = I on the mp x mp square, 0 on the rows below it (bordered layout, leading dimension mr): what the tiles' products add to
__global__ void fitc_init_b_kernel(double* B, int64_t mr, int64_t mp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i < mr) B[i + j * mr] = i == j ? 1.0 : 0.0;
}
// ... and after them: the columns m .. mp - 1 belong to no inducing point (the products wrote the border row's share there when m
// is no multiple of the tile): identity again, so that the padded factor stays trivial
__global__ void fitc_fix_b_kernel(double* B, int64_t mr, int64_t m) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, j = m + blockIdx.y;
  if (i < mr) B[i + j * mr] = i == j ? 1.0 : 0.0;
}

// ---- pass 2: the gradient ------------------------------------------------------------------------------------------------------
struct FitcRowArgs {
  const double* At;  // A^T of the tile (V layout)
  double* Ct;        // C^T = A^T L_B^-T in, Lambda^-1 C^T out
  int64_t ldt, tc;
  int32_t m;
  const double* w;   // L_B^-T c (= A alpha)
  const double* y;   // of the tile's first column on (as lam, alpha, d, part)
  const double* lam;
  double* alpha;     // (y - A^T w) / lambda
  double* d;         // 1 / lambda - colsumsq(C) / lambda^2 - alpha^2: the diagonal of S^-1 - alpha alpha^T
  double* part;      // slot 2 of [block of 32 columns][FITC_COL_SUMS]: sum d
};

__global__ __launch_bounds__(256) void fitc_row_kernel(FitcRowArgs a) {
  __shared__ double rp[8][32], cp[8][32];
  __shared__ double il[32], dsum[32];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t n = (int64_t)blockIdx.x * FITC_COL_BLOCK + tx;
  const bool real = n < a.tc;
  double r = 0.0, cs = 0.0;
  if (real)
    for (int k = ty; k < a.m; k += 8) {
      r = fma(a.At[n + (int64_t)k * a.ldt], a.w[k], r);
      const double c = a.Ct[n + (int64_t)k * a.ldt];
      cs = fma(c, c, cs);
    }
  rp[ty][tx] = r;
  cp[ty][tx] = cs;
  __syncthreads();
  if (ty == 0) {
    double inv = 0.0, dn = 0.0;
    if (real) {
      double rr = rp[0][tx], cc = cp[0][tx];
#pragma unroll
      for (int j = 1; j < 8; ++j) rr += rp[j][tx], cc += cp[j][tx];
      inv = 1.0 / a.lam[n];
      const double al = (a.y[n] - rr) * inv;
      dn = inv - cc * inv * inv - al * al;
      a.alpha[n] = al;
      a.d[n] = dn;
    }
    il[tx] = inv;
    dsum[tx] = dn;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int j = 0; j < 32; ++j) s += dsum[j];
    a.part[(int64_t)blockIdx.x * FITC_COL_SUMS + 2] = s;
  }
  if (real)
    for (int k = ty; k < a.m; k += 8) a.Ct[n + (int64_t)k * a.ldt] *= il[tx];
}

// T^T = H^T - alpha w^T - diag(d) A^T in place of H^T; 0 on the padding (the transposes and the GEMM behind it read all of it).
// grid (tpad / 256, mp)
__global__ __launch_bounds__(256) void fitc_adjoint_kernel(double* Ht, const double* __restrict__ At, int64_t ldt, int64_t tc, int32_t m,
                                                           const double* __restrict__ alpha, const double* __restrict__ d,
                                                           const double* __restrict__ w) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y;
  if (n >= ldt) return;
  double v = 0.0;
  if (n < tc && k < m) v = Ht[n + (int64_t)k * ldt] - alpha[n] * w[k] - d[n] * At[n + (int64_t)k * ldt];
  Ht[n + (int64_t)k * ldt] = v;
}

// sum_{i, j} G[i + j * ldg] dk(p_i, q_j) / dtheta over a rectangle of ti x tj tiles of 128 x 128 pairs, P the rows (fast index of G)
// and Q the columns, both prepared point sets of the SAME lengthscales.  Stationary kernels only: with u_c = (p_c - q_c) / ls_c,
//   dk / d ls_c = eta^2 f'(r^2) (-2 u_c^2 / ls_c)        dk / d eta = 2 k / eta
// so a pair adds g eta^2 f'(r^2) u_c^2 to slot c < NC and g eta^2 f(r^2) to slot NC; the host applies -2 / ls_c and 2 / eta.
// One workgroup per tile, as cov_general_tile stages it; a thread owns row il of the tile and half of its columns.  Its NC + 1
// sums go through a wave reduction in a fixed lane order, the four waves are added in order, and the workgroup WRITES its vector
// to part[block * FITC_DERIV_SUMS ..]; fitc_fold_kernel adds the workgroups.
struct FitcDerivArgs {
  CovParams p;
  PointSet rows, cols;
  const double* G;
  int64_t ldg;
  int32_t ti, tj;
  double* part;
};

template <int KIND, int NC>
__global__ __launch_bounds__(256) void fitc_deriv_kernel(FitcDerivArgs a) {
  __shared__ double xj[NC][TILE];
  __shared__ double wred[4][NC + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tix = (int)(blockIdx.x % (unsigned)a.ti), tjx = (int)(blockIdx.x / (unsigned)a.ti);
  const int64_t gi0 = (int64_t)tix * TILE, gj0 = (int64_t)tjx * TILE;
  const int il = tid & (TILE - 1), jh = tid >> 7;
  const int64_t gi = gi0 + il;
  for (int idx = tid; idx < NC * TILE; idx += 256) {
    const int k = idx / TILE, j = idx - k * TILE;
    xj[k][j] = a.cols.xs[(int64_t)k * a.cols.npad + gj0 + j];
  }
  double xi[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) xi[k] = a.rows.xs[(int64_t)k * a.rows.npad + gi];
  __syncthreads();
  double acc[NC + 1];
#pragma unroll
  for (int k = 0; k <= NC; ++k) acc[k] = 0.0;
  if (gi < a.rows.n) {
    const double* g = a.G + gi + (gj0 + jh * (TILE / 2)) * a.ldg;
    for (int jj = 0; jj < TILE / 2; ++jj) {
      const int j = jh * (TILE / 2) + jj;
      if (gj0 + j >= a.cols.n) break;  // (the real columns come first)
      double u2[NC];
      double r2 = 0.0;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const double u = xi[k] - xj[k][j];
        u2[k] = u * u;
        r2 += u2[k];
      }
      const double gv = g[(int64_t)jj * a.ldg];
      const double gk = gv * (a.p.eta2 * stationary_dr2<KIND>(r2));
#pragma unroll
      for (int k = 0; k < NC; ++k) acc[k] = fma(gk, u2[k], acc[k]);
      acc[NC] = fma(gv, a.p.eta2 * stationary<KIND>(r2), acc[NC]);
    }
  }
#pragma unroll
  for (int k = 0; k <= NC; ++k) {
    double s = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if (lane == 0) wred[wave][k] = s;
  }
  __syncthreads();
  if (tid < FITC_DERIV_SUMS) {
    // slots: [0, NC) the lengthscale sums, [16] eta; what lies between is written 0
    const int src = tid < NC ? tid : (tid == FITC_DERIV_SUMS - 1 ? NC : -1);
    const double s = src < 0 ? 0.0 : ((wred[0][src] + wred[1][src]) + wred[2][src]) + wred[3][src];
    a.part[(int64_t)blockIdx.x * FITC_DERIV_SUMS + tid] = s;
  }
}

// ---- prediction ----------------------------------------------------------------------------------------------------------------
// As^T (mpad x m, test index fastest) and C*^T = As^T L_B^-T -> mean_n = sum_k As[k, n] w_k,
// var_n = k**_n - sum_k As[k, n]^2 + sum_k C*[k, n]^2  (kss carries the noise when it was asked for).  A thread per test point,
// the inducing index in ascending order: a point's result does not depend on where in the call it stands.
__global__ __launch_bounds__(256) void fitc_predict_kernel(const double* __restrict__ As, const double* __restrict__ Cs, int64_t ld, int64_t mc,
                                                           int32_t m, const double* __restrict__ w, const double* __restrict__ kss,
                                                           double* __restrict__ mean, double* __restrict__ var) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= mc) return;
  double mu = 0.0, s1 = 0.0, s2 = 0.0;
  for (int k = 0; k < m; ++k) {
    const double a = As[n + (int64_t)k * ld], c = Cs[n + (int64_t)k * ld];
    mu = fma(a, w[k], mu);
    s1 = fma(a, a, s1);
    s2 = fma(c, c, s2);
  }
  mean[n] = mu;
  var[n] = (kss[n] - s1) + s2;
}

}  // namespace gmb
