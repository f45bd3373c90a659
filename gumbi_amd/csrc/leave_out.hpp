// leave_out.hpp -- what the fitted model predicts for training rows it is NOT shown, from the resident factorisation alone.
//
// For a GP at fixed hyper-parameters (Rasmussen & Williams 5.4.2), with Sigma = L L^T the resident factorisation (noise AND jitter
// on its diagonal), alpha = Sigma^-1 y and B a set of training rows,
//
//   y_B | y_-B ~ N( y_B - C^-1 alpha_B , C^-1 ),   C = (Sigma^-1)_BB          one row:  mu_-i = y_i - alpha_i / d_i,  1 / d_i,
//                                                                              d_i = (Sigma^-1)_ii
//
// -- no refit, no second factorisation of anything of order N.  Sigma holds the jitter, gmb_predict's variances do not, so every
// variance here has the jitter taken off again (and the row's noise too when the caller asks for the latent function's).
//
//   gmb_loo, product form    behind a tile-path gradient U = L^-T is resident (predict_form.hpp) and d_i = sum_{j >= i} U_ij^2:
//                            loo_u_rowsumsq_kernel, ONE pass over the triangle, + loo_u_final_kernel with the gradient's alpha
//   gmb_loo, solve form      selection rows e_i solved against L (the prediction's own solve): row j of V = column i of L^-1, so
//                            <V_j, v> = alpha_i and |V_j|^2 = d_i by predict_partial_kernel; loo_solve_final_kernel
//   gmb_leave_out            the same solve for the rows of B, C = V V^T on the joint posterior's second matrix, R R^T = C by the
//                            engine's Cholesky, X = R^-T, then var = rowsumsq(X), mean = y_B - X (X^T g): lo_xt_g_kernel,
//                            predict_partial_kernel on X, lo_group_final_kernel
//
// Every sum has a fixed order and nothing is accumulated with atomics: the same bits call after call.  The index check at the top
// has no HIP in it (LEAVE_OUT_HOST_ONLY leaves the kernels out), so tools/leave_out_check.cpp runs it on the host.
#pragma once
#include <stdint.h>

#include <vector>

namespace gmb {

// What gmb_leave_out asks of idx[0 .. m): 1 <= m <= N, every entry in [0, N), no entry twice.
//   0 fine | 1 idx null or m out of range | 2 idx[*pos] out of range | 3 idx[*pos] repeats an earlier entry
inline int leave_out_check_indices(const int64_t* idx, int64_t m, int64_t N, int64_t* pos) {
  if (pos) *pos = -1;
  if (!idx || N < 1 || m < 1 || m > N) return 1;
  std::vector<unsigned char> seen((size_t)N, 0);
  for (int64_t j = 0; j < m; ++j) {
    const int64_t i = idx[j];
    if (i < 0 || i >= N) {
      if (pos) *pos = j;
      return 2;
    }
    if (seen[(size_t)i]) {
      if (pos) *pos = j;
      return 3;
    }
    seen[(size_t)i] = 1;
  }
  return 0;
}

}  // namespace gmb

#ifndef LEAVE_OUT_HOST_ONLY
#include <hip/hip_runtime.h>

#include "gemm_f64.hpp"

namespace gmb {

// the model's noise variance at training row i: sigma^2, times the row's output level's multiplier for heteroscedastic outputs
// (`cat`: the output table's row of the resident prepared points, null without one -- term 0's preparation, covariance.hpp)
struct NoiseAt {
  double sigma2;
  const double* mult;
  const int32_t* cat;
  __device__ __forceinline__ double operator()(int64_t i) const { return cat ? sigma2 * mult[cat[i]] : sigma2; }
};

// what is taken off 1 / d_i (or off a diagonal entry of C^-1): the jitter always, the row's noise for the latent function
struct LeaveOutDiag {
  NoiseAt noise;
  double jitter;
  int32_t with_noise;
  __device__ __forceinline__ double operator()(int64_t i) const { return jitter + (with_noise ? 0.0 : noise(i)); }
};

// V[j + col_j * ldv] = 1, col_j = idx ? idx[j] : i0 + j, j < count: selection rows (or, idx null and i0 = 0, the identity) on a
// cleared buffer
__global__ __launch_bounds__(256) void lo_scatter_kernel(double* __restrict__ V, int64_t ldv, const int64_t* __restrict__ idx,
                                                         int64_t i0, int64_t count) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= count) return;
  const int64_t col = idx ? idx[j] : i0 + j;
  V[j + col * ldv] = 1.0;
}

// ---- gmb_loo, product form ---------------------------------------------------------------------------------------------------
struct LooUArgs {
  const double* U;      // U(i, j), i < j, at U + i + j * ldu for the tiles strictly above the diagonal (the factor buffer)
  int64_t ldu;          // even (the loads are two rows wide)
  const double* udiag;  // tile (r, r) at udiag + r * 128 * 128, leading dimension 128
  int64_t n;            // columns >= n are padding and do not enter
  int32_t nct;          // block columns
  int32_t r0;           // first block row of the launch (blockIdx.y = 0)
  double* part;         // part[chunk * np + i] = sum over the chunk's columns of U(i, j)^2
  int64_t np;
};

constexpr int LOO_CH = 2;  // block columns per workgroup: 256 KiB of U

// d_i = sum_{i <= j < n} U(i, j)^2 in two stages.  Workgroup (chunk, r) owns block row r0 + r and the block columns
// r + LOO_CH chunk ... of it, counted from the diagonal tile; the row index is the fast one in memory, so threads run along i:
// lane l of every wave holds rows 2 l and 2 l + 1 (one 16 B load per column, a 1 KiB segment per wave), wave w the columns
// w, w + 4, ... of each tile, eight loads in flight per lane.  The four waves' sums meet in LDS and are added in wave order.  The
// triangle is ragged -- block row r has nct - r tiles -- and the grid's y index is the block row, so the long rows are
// dispatched first; workgroups beyond a row's last chunk leave at once (loo_u_final_kernel does not read their partials).
__global__ __launch_bounds__(256) void loo_u_rowsumsq_kernel(LooUArgs a) {
  __shared__ double red[4][TILE];
  const int r = a.r0 + (int)blockIdx.y;
  const int ct0 = r + (int)blockIdx.x * LOO_CH;
  if (ct0 >= a.nct) return;
  const int ct1 = ct0 + LOO_CH < a.nct ? ct0 + LOO_CH : a.nct;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int il = 2 * lane;
  const int64_t i = (int64_t)r * TILE + il;
  double s0 = 0.0, s1 = 0.0;
  for (int ct = ct0; ct < ct1; ++ct) {
    const int64_t j0 = (int64_t)ct * TILE;
    const int jn = a.n - j0 < TILE ? (int)(a.n - j0) : TILE;  // (<= 0 cannot happen: ct < nct = ceil(n / 128))
    if (ct == r) {  // the diagonal tile: its own buffer, and only il <= jl is U
      const double* src = a.udiag + (int64_t)r * TILE * TILE + il;
      for (int jl = wave; jl < jn; jl += 4) {
        const d2 x = *reinterpret_cast<const d2*>(src + (int64_t)jl * TILE);
        if (il <= jl) s0 = fma(x[0], x[0], s0);
        if (il + 1 <= jl) s1 = fma(x[1], x[1], s1);
      }
    } else {
      const double* src = a.U + i + j0 * a.ldu;
#pragma unroll 8
      for (int jl = wave; jl < jn; jl += 4) {
        const d2 x = *reinterpret_cast<const d2*>(src + (int64_t)jl * a.ldu);
        s0 = fma(x[0], x[0], s0);
        s1 = fma(x[1], x[1], s1);
      }
    }
  }
  red[wave][il] = s0;
  red[wave][il + 1] = s1;
  __syncthreads();
  if (threadIdx.x < TILE) {
    const int t = threadIdx.x;
    a.part[(int64_t)blockIdx.x * a.np + (int64_t)r * TILE + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  }
}

// row i = i0 + j, j < n: d_i = its chunk partials in chunk order, then mean and variance from the gradient's alpha
__global__ __launch_bounds__(256) void loo_u_final_kernel(const double* __restrict__ part, int64_t np, int32_t nct, int64_t i0, int64_t n,
                                                          const double* __restrict__ alpha, const double* __restrict__ y, LeaveOutDiag off,
                                                          double* __restrict__ mean, double* __restrict__ var) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int64_t i = i0 + j;
  const int nchunk = (nct - (int)(i / TILE) + LOO_CH - 1) / LOO_CH;
  double d = 0.0;
  for (int c = 0; c < nchunk; ++c) d += part[(int64_t)c * np + i];
  mean[j] = y[i] - alpha[i] / d;
  var[j] = 1.0 / d - off(i);
}

// ---- gmb_loo, solve form: behind predict_partial_kernel on the solved selection rows (part_mu: <V_j, v> = alpha_i, part_s: d_i) ---
__global__ __launch_bounds__(256) void loo_solve_final_kernel(const double* __restrict__ part_mu, const double* __restrict__ part_s, int nchunk,
                                                              int64_t mpad, int64_t i0, int64_t n, const double* __restrict__ y,
                                                              LeaveOutDiag off, double* __restrict__ mean, double* __restrict__ var) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  double am = 0.0, d = 0.0;
  for (int c = 0; c < nchunk; ++c) {
    am += part_mu[(int64_t)c * mpad + j];
    d += part_s[(int64_t)c * mpad + j];
  }
  const int64_t i = i0 + j;
  mean[j] = y[i] - am / d;
  var[j] = 1.0 / d - off(i);
}

// ---- gmb_leave_out -------------------------------------------------------------------------------------------------------------
// C(j, j) = 1 for m <= j < mp: the padding of the second matrix, as the covariance build leaves it
__global__ __launch_bounds__(128) void lo_pad_diag_kernel(double* __restrict__ Cm, int64_t ldc, int64_t m, int64_t mp) {
  const int64_t j = m + (int64_t)blockIdx.x * 128 + threadIdx.x;
  if (j < mp) Cm[j + j * ldc] = 1.0;
}

// t_j = sum_{i <= j} X(i, j) g_i for column j = blockIdx.x of the upper-triangular X = R^-T (row index fastest): 256 threads take
// the rows t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void lo_xt_g_kernel(const double* __restrict__ X, int64_t ldx, const double* __restrict__ g,
                                                      double* __restrict__ t) {
  __shared__ double red[4];
  const int64_t j = blockIdx.x;
  const double* col = X + j * ldx;
  double as = 0.0;
  for (int64_t i = threadIdx.x; i <= j; i += 256) as = fma(col[i], g[i], as);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) as += __shfl_down(as, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = as;
  __syncthreads();
  if (threadIdx.x == 0) t[j] = (red[0] + red[1]) + (red[2] + red[3]);
}

// behind predict_partial_kernel on X with t in v's place (part_mu: (X t)_j = (C^-1 g)_j, part_s: (C^-1)_jj), outputs in idx's order
__global__ __launch_bounds__(256) void lo_group_final_kernel(const double* __restrict__ part_mu, const double* __restrict__ part_s, int nchunk,
                                                             int64_t mpad, int64_t m, const int64_t* __restrict__ idx,
                                                             const double* __restrict__ y, LeaveOutDiag off, double* __restrict__ mean,
                                                             double* __restrict__ var) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  double am = 0.0, as = 0.0;
  for (int c = 0; c < nchunk; ++c) {
    am += part_mu[(int64_t)c * mpad + j];
    as += part_s[(int64_t)c * mpad + j];
  }
  const int64_t i = idx[j];
  mean[j] = y[i] - am;
  var[j] = as - off(i);
}

// the same correction on the diagonal of the symmetrised row-major C^-1
__global__ __launch_bounds__(256) void lo_cov_diag_kernel(double* __restrict__ out, int64_t ldo, int64_t m, const int64_t* __restrict__ idx,
                                                          LeaveOutDiag off) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < m) out[j * ldo + j] -= off(idx[j]);
}

}  // namespace gmb
#endif  // LEAVE_OUT_HOST_ONLY
