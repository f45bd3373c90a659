// predict_terms.hpp -- the posterior of an additive model's components, all of them from one pass.
//
// With L, v = L^-1 y of the WHOLE model and V_t = K_t(X*, X) L^-T for term t, per test point x*:
//   mu_t            = <V_t, v>
//   cov(f_t, f_u|y) = delta_tu k_t(x*, x*) - <V_t, V_u>        (the priors of different terms are independent)
// gmb_predict_decompose stacks the T blocks V_t on top of each other -- (T mpad) x Np doubles, test index fastest, term t in
// rows [t mpad, (t + 1) mpad) -- solves them in ONE triangular solve and reduces them here: T means and the T (T + 1) / 2 inner
// products per test point, in two deterministic stages like the prediction's own (covariance.hpp: predict_partial_kernel).
// No atomics, every output written once.
#pragma once
#include "covariance.hpp"
#include "workspace_sizes.hpp"  // TG_MAX_TERMS, tg_entries

namespace gmb {

// part[chunk][q][m]: q < NT the chunk's share of mu_q, q = NT + p the chunk's share of <V_t, V_u>.
// Grid (ceil(mpad / 256), nchunk), 256 threads, one test point per thread; the chunk's RED_CHUNK entries of v sit in LDS.  Every
// load of V is a run of 256 consecutive doubles across the workgroup; a thread reads its NT values of training row i, then
// all its fmas of that row, in ascending i.
template <int NT>
__global__ __launch_bounds__(256) void term_gram_partial_kernel(const double* __restrict__ V, int64_t ldz, int64_t mpad,
                                                                const double* __restrict__ v, int64_t n, double* __restrict__ part) {
  constexpr int NQ = tg_entries(NT);
  __shared__ double vs[RED_CHUNK];
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.y * RED_CHUNK;
  const int64_t i1 = (i0 + RED_CHUNK < n) ? i0 + RED_CHUNK : n;
  if (i0 + threadIdx.x < n) vs[threadIdx.x] = v[i0 + threadIdx.x];
  __syncthreads();
  if (m >= mpad) return;  // mpad is a multiple of 128, the block covers 256
  double mu[NT], g[NT * (NT + 1) / 2];
#pragma unroll
  for (int t = 0; t < NT; ++t) mu[t] = 0.0;
#pragma unroll
  for (int p = 0; p < NT * (NT + 1) / 2; ++p) g[p] = 0.0;
  const double* col = V + m + i0 * ldz;
  for (int64_t i = i0; i < i1; ++i) {
    double x[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) x[t] = col[(int64_t)t * mpad];
    const double vi = vs[i - i0];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      mu[t] = fma(x[t], vi, mu[t]);
#pragma unroll
      for (int u = 0; u <= t; ++u) g[t * (t + 1) / 2 + u] = fma(x[t], x[u], g[t * (t + 1) / 2 + u]);
    }
    col += ldz;
  }
  double* out = part + (int64_t)blockIdx.y * NQ * mpad + m;
#pragma unroll
  for (int t = 0; t < NT; ++t) out[(int64_t)t * mpad] = mu[t];
#pragma unroll
  for (int p = 0; p < NT * (NT + 1) / 2; ++p) out[(int64_t)(NT + p) * mpad] = g[p];
}

// The chunks added in chunk order: means[t][m] = mu_t, cov[p][m] = delta_tu kss_t - <V_t, V_u> (kss: nt rows of mpad, the
// terms' prior variances without noise).  One thread per test point and entry: grid (ceil(mc / 256), tg_entries(nt)).
__global__ __launch_bounds__(256) void term_gram_final_kernel(const double* __restrict__ part, int nchunk, int nt, int64_t mpad,
                                                              const double* __restrict__ kss, int64_t mc, double* __restrict__ means,
                                                              double* __restrict__ cov) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int q = (int)blockIdx.y, nq = tg_entries(nt);
  if (m >= mc || q >= nq) return;
  double acc = 0.0;
  for (int c = 0; c < nchunk; ++c) acc += part[((int64_t)c * nq + q) * mpad + m];
  if (q < nt) {
    means[(int64_t)q * mpad + m] = acc;
    return;
  }
  const int p = q - nt;
  int t = 0;
  while ((t + 1) * (t + 2) / 2 <= p) ++t;  // row t of the packed triangle holds p = t (t + 1) / 2 .. t (t + 1) / 2 + t
  const int u = p - t * (t + 1) / 2;
  cov[(int64_t)p * mpad + m] = (t == u ? kss[(int64_t)t * mpad + m] : 0.0) - acc;
}

// the model's noise variance at prepared test points: sigma^2 (x the output level's multiplier) -- what with_noise adds to a
// variance.  `p`, and the preparation of `pts`, are term 0's.
__global__ __launch_bounds__(256) void term_noise_kernel(CovParams p, PointSet pts, double* __restrict__ noise) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= pts.n) return;
  double nz = p.sigma2;
  if (p.noise_tab >= 0) nz *= p.noise_mult[pts.cat[(int64_t)p.noise_tab * pts.npad + m]];
  noise[m] = nz;
}

}  // namespace gmb
