// laplace.hpp -- the kernels of GP classification by the Laplace approximation that are its own.  Rasmussen &
// Williams, Algorithms 3.1, 3.2 and 5.1 for a Bernoulli likelihood with a logit link, labels y in {0, 1}, zero mean:
//
//   pi = 1 / (1 + e^-f)    log p(y | f) = sum y f - log(1 + e^f)    g = y - pi    W = pi (1 - pi)    s = sqrt(W)
//   Newton:  b = W f + g    B = I + (s s^T) o Sigma = L L^T    a^ = b - s o B^-1 (s o (Sigma b))    a <- a + t (a^ - a)    f = Sigma a
//   Psi(a, f) = -1/2 a^T f + log p(y | f)      -log q(y | theta) = -Psi(a^, f^) + sum log L_ii
//   gradient:  R = (s s^T) o B^-1    s2 = -1/2 (1 - diag B^-1)(1 - 2 pi)    u = s2 - R (Sigma s2)
//              d(-log q)/d theta = 1/2 tr((Z' - a' a'^T) dSigma/d theta),  Z' = R + u u^T,  a' = a^ + u   (the trace pass of the exact path)
//   predict:   mean = k*^T (y - pi^)    var = k** - |L^-1 (s o k*)|^2
//
// Resident N x N matrices: Sigma (the Laplace state's own buffer), the factor buffer (B, then L) and the inverse's (B^-1, then Z'):
// the exact path's two plus one.  The covariance build, the Cholesky, the triangular solves, the inverse and the trace pass are the
// engine's; here are
//   laplace_lik_kernel     one pass over N: pi, W, s, g, b from f and y, and per workgroup the terms of Psi, max |f_new - f|,
//                          max |f_new| and the count of labels that are neither 0 nor 1
//   laplace_fold_kernel    the fixed-order second stage of those partial sets
//   symv_lower_kernel      out = A v from the lower triangle of A in 128 x 128 tiles: every tile writes its two partial vectors to a
//   symv_sum_kernel        slot of its own (laplace_plan.hpp), the second launch adds the slots of a block row in a fixed order
//   laplace_scale_kernel   B = I + (s s^T) o Sigma into the factor buffer (lower triangle, the right-hand side in the border row,
//                          identity on the padding); in place on B^-1: Z' = (s s^T) o B^-1 + u u^T
//   the vector kernels     a^ and the damped step; s2 from diag B^-1; u and a'; s o x; the prediction's column scaling
// Every sum has a fixed order and there is no floating-point atomic: the same bits call after call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "laplace_plan.hpp"

namespace gmb {

// ---- the likelihood pass -------------------------------------------------------------------------------------------------------
struct LaplaceLikArgs {
  const double* fnew;  // the iterate the quantities are formed at
  const double* fold;  // the previous one (max |f_new - f|)
  const double* a;     // f_new = Sigma a (the quadratic term of Psi)
  const double* y;
  int64_t n, np;
  double *pi, *W, *s, *g, *b;  // np each; 0 on the padding
  double* part;        // [workgroup][LAP_LIK_SUMS]
};

// pi, W and log(1 + e^f) from e^-|f|: nothing overflows and nothing cancels at |f| = 60, and W underflows to an exact 0 beyond |f| ~ 745
__global__ __launch_bounds__(LAP_LIK_BLOCK) void laplace_lik_kernel(LaplaceLikArgs k) {
  __shared__ double red[LAP_LIK_SUMS][LAP_LIK_BLOCK];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * LAP_LIK_BLOCK + tid;
  double lp = 0.0, af = 0.0, df = 0.0, fm = 0.0, bad = 0.0, nonfin = 0.0;
  if (i < k.np) {
    double pi = 0.0, W = 0.0, s = 0.0, g = 0.0, b = 0.0;
    if (i < k.n) {
      const double f = k.fnew[i], y = k.y[i];
      const double e = exp(-fabs(f));
      const double r = 1.0 / (1.0 + e);
      pi = f >= 0.0 ? r : e * r;
      W = e * r * r;
      s = sqrt(W);
      g = y - pi;
      b = fma(W, f, g);
      lp = y * f - (fmax(f, 0.0) + log1p(e));
      af = k.a[i] * f;
      df = fabs(f - k.fold[i]);
      fm = fabs(f);
      bad = (y == 0.0 || y == 1.0) ? 0.0 : 1.0;
      nonfin = isfinite(f) ? 0.0 : 1.0;
    }
    k.pi[i] = pi, k.W[i] = W, k.s[i] = s, k.g[i] = g, k.b[i] = b;
  }
  red[0][tid] = lp, red[1][tid] = af, red[2][tid] = df, red[3][tid] = fm, red[4][tid] = bad, red[5][tid] = nonfin;
  __syncthreads();
  for (int off = LAP_LIK_BLOCK / 2; off > 0; off >>= 1) {
    if (tid < off) {
      red[0][tid] += red[0][tid + off];
      red[1][tid] += red[1][tid + off];
      red[2][tid] = fmax(red[2][tid], red[2][tid + off]);
      red[3][tid] = fmax(red[3][tid], red[3][tid + off]);
      red[4][tid] += red[4][tid + off];
      red[5][tid] += red[5][tid + off];
    }
    __syncthreads();
  }
  if (tid < LAP_LIK_SUMS) k.part[(int64_t)blockIdx.x * LAP_LIK_SUMS + tid] = red[tid][0];
}

// out[q] = the partial sets' q-th entries added (q = 2, 3: their maximum): ONE workgroup; thread t takes the blocks t, t + 256, ...
// in ascending order, then a fixed LDS tree
__global__ __launch_bounds__(256) void laplace_fold_kernel(const double* __restrict__ part, int64_t nblocks, double* __restrict__ out) {
  __shared__ double red[256];
  for (int q = 0; q < LAP_LIK_SUMS; ++q) {
    const bool is_max = q == 2 || q == 3;
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < nblocks; b += 256) {
      const double v = part[b * LAP_LIK_SUMS + q];
      s = is_max ? fmax(s, v) : s + v;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if ((int)threadIdx.x < off) red[threadIdx.x] = is_max ? fmax(red[threadIdx.x], red[threadIdx.x + off]) : red[threadIdx.x] + red[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[q] = red[0];
    __syncthreads();
  }
}

// ---- out = A v from the lower triangle -----------------------------------------------------------------------------------------
// grid (nt, nt), workgroup (I, J) = (blockIdx.x, blockIdx.y) with J <= I; 256 threads: thread t owns row i = t & 127 of the tile
// and the columns [64 h, 64 h + 64), h = t >> 7.  Its row sum stays in a register (the two halves are added in order through LDS);
// a column's sum over the 128 rows is two wave reductions in a fixed lane order, added in order.  Elements with a row or column
// index >= n are read as 0 (the border row of the factor layout and the padding never enter), a diagonal tile gives its elements
// i >= j to the row part and i > j to the column part.
__global__ __launch_bounds__(256) void symv_lower_kernel(const double* __restrict__ A, int64_t ld, int64_t n, const double* __restrict__ v,
                                                         double* __restrict__ ws) {
  const int I = blockIdx.x, J = blockIdx.y;
  if (J > I) return;
  __shared__ double vi[LAP_TILE], vj[LAP_TILE];
  __shared__ double rowh[2][LAP_TILE];
  __shared__ double colw[2][LAP_TILE];
  const int tid = threadIdx.x, il = tid & (LAP_TILE - 1), h = tid >> 7, lane = tid & 63, wv = (tid >> 6) & 1;
  const int64_t gi0 = (int64_t)I * LAP_TILE, gj0 = (int64_t)J * LAP_TILE;
  if (tid < LAP_TILE) vi[tid] = gi0 + tid < n ? v[gi0 + tid] : 0.0;
  else vj[tid - LAP_TILE] = gj0 + (tid - LAP_TILE) < n ? v[gj0 + (tid - LAP_TILE)] : 0.0;
  __syncthreads();
  const int64_t gi = gi0 + il;
  const bool diag = I == J;
  const double my_v = vi[il];
  const double* col = A + gi + (gj0 + (int64_t)h * 64) * ld;
  double racc = 0.0;
  for (int jj = 0; jj < 64; ++jj) {
    const int j = h * 64 + jj;
    double x = 0.0;
    if (gi < n && gj0 + j < n && (!diag || j <= il)) x = col[(int64_t)jj * ld];
    racc = fma(x, vj[j], racc);
    double c = (diag && j == il) ? 0.0 : x * my_v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if (lane == 0) colw[wv][j] = c;
  }
  rowh[h][il] = racc;
  __syncthreads();
  double* slot = ws + lap_slot(I, J) * LAP_SLOT;
  if (tid < LAP_TILE) slot[tid] = rowh[0][tid] + rowh[1][tid];
  else slot[tid] = colw[0][tid - LAP_TILE] + colw[1][tid - LAP_TILE];
}

// block row R: its nt + 1 parts in the plan's order; 0 at and beyond row n.  grid nt, 128 threads.
__global__ __launch_bounds__(LAP_TILE) void symv_sum_kernel(const double* __restrict__ ws, int64_t nt, int64_t n, double* __restrict__ out) {
  const int64_t R = blockIdx.x, i = R * LAP_TILE + threadIdx.x;
  double s = 0.0;
  for (int64_t q = 0; q < lap_terms(nt); ++q) s += ws[lap_term_offset(R, q) + threadIdx.x];
  out[i] = i < n ? s : 0.0;
}

// ---- B and Z' ------------------------------------------------------------------------------------------------------------------
// mode 0: out(i, j) = [i == j] + s_i s_j src(i, j) for j <= i < n; row n (the border row of the bordered layout) = rhs (or 0);
//         everything else of the lower triangle of the nr x np layout: the identity.  src = Sigma, out = the factor buffer.
// mode 1: out(i, j) = s_i s_j out(i, j) + u_i u_j for j <= i < n, 0 on the rest of the lower triangle of the np x np matrix.
// grid (np, rows / 256): a thread per element of column blockIdx.x, the row index fastest.
struct LaplaceScaleArgs {
  const double* src;
  int64_t lds;
  double* out;
  int64_t ldo;
  int64_t n, rows;  // rows of the layout written: nr (mode 0) or np (mode 1)
  const double* s;
  const double* u;    // mode 1
  const double* rhs;  // mode 0: the border row, or null
  int mode;
};
__global__ __launch_bounds__(256) void laplace_scale_kernel(LaplaceScaleArgs k) {
  const int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x, j = blockIdx.x;
  if (i >= k.rows || i < j) return;
  double v;
  if (k.mode == 0) {
    if (i < k.n && j < k.n) v = fma(k.s[i] * k.s[j], k.src[i + j * k.lds], i == j ? 1.0 : 0.0);
    else if (i == k.n && j < k.n) v = k.rhs ? k.rhs[j] : 0.0;
    else v = i == j ? 1.0 : 0.0;
  } else {
    v = (i < k.n && j < k.n) ? fma(k.s[i] * k.s[j], k.out[i + j * k.ldo], k.u[i] * k.u[j]) : 0.0;
  }
  k.out[i + j * k.ldo] = v;
}

// ---- vector kernels (a thread per entry, np entries, 0 on the padding) ----------------------------------------------------------
// out = s o x
__global__ void laplace_mul_kernel(const double* __restrict__ s, const double* __restrict__ x, int64_t n, int64_t np, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < np) out[i] = i < n ? s[i] * x[i] : 0.0;
}
// a^ = b - s o w (w = B^-1 (s o Sigma b)), and the full step's candidate a_c = a + t (a^ - a)
__global__ void laplace_ahat_kernel(const double* __restrict__ b, const double* __restrict__ s, const double* __restrict__ w,
                                    const double* __restrict__ a, double t, int64_t n, int64_t np, double* __restrict__ ah,
                                    double* __restrict__ ac) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  double h = 0.0, c = 0.0;
  if (i < n) {
    h = fma(-s[i], w[i], b[i]);
    c = fma(t, h - a[i], a[i]);
  }
  ah[i] = h, ac[i] = c;
}
// a_c = a + t (a^ - a) alone: a halved step
__global__ void laplace_step_kernel(const double* __restrict__ a, const double* __restrict__ ah, double t, int64_t n, int64_t np,
                                    double* __restrict__ ac) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < np) ac[i] = i < n ? fma(t, ah[i] - a[i], a[i]) : 0.0;
}
// s2 = -1/2 (1 - (B^-1)_ii)(1 - 2 pi_i): the posterior variance (1 - B^-1_ii) / W_i times 1/2 d^3 log p / df^3 = -1/2 W_i (1 - 2 pi_i)
// with W cancelled -- no division, valid where W_i is 0
__global__ void laplace_s2_kernel(const double* __restrict__ Binv, int64_t ld, const double* __restrict__ pi, int64_t n, int64_t np,
                                  double* __restrict__ s2) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < np) s2[i] = i < n ? -0.5 * (1.0 - Binv[i * (ld + 1)]) * (1.0 - 2.0 * pi[i]) : 0.0;
}
// u = s2 - s o r (r = B^-1 (s o Sigma s2)), and a' = a^ + u
__global__ void laplace_u_kernel(const double* __restrict__ s2, const double* __restrict__ s, const double* __restrict__ r,
                                 const double* __restrict__ a, int64_t n, int64_t np, double* __restrict__ u, double* __restrict__ ap) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  double uu = 0.0, p = 0.0;
  if (i < n) {
    uu = fma(-s[i], r[i], s2[i]);
    p = a[i] + uu;
  }
  u[i] = uu, ap[i] = p;
}

// ---- prediction ----------------------------------------------------------------------------------------------------------------
// V = K(X*, X) (mpad x np, the test index fastest): V[m, k] <- V[m, k] s_k for the solve against L, behind the mean k*^T g, which
// the prediction's own reduction takes from the unscaled V.  grid (mpad / 256, chunks of LAP_SCALE_COLS columns).
constexpr int LAP_SCALE_COLS = 256;
__global__ __launch_bounds__(256) void laplace_colscale_kernel(double* __restrict__ V, int64_t mpad, int64_t n, const double* __restrict__ s) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= mpad) return;
  const int64_t k0 = (int64_t)blockIdx.y * LAP_SCALE_COLS, k1 = k0 + LAP_SCALE_COLS < n ? k0 + LAP_SCALE_COLS : n;
  for (int64_t k = k0; k < k1; ++k) V[m + k * mpad] *= s[k];
}

}  // namespace gmb
