// design_batch.hpp -- the greedy loop of gmb_design_batch: integrated variance reduction over a reference set,
// q picks as q rank-1 downdates of the rectangular posterior covariance D = C(candidates, [candidates; reference points]).
//
// D is stored a candidate per row (design_plan.hpp: the stacked point index fastest, `ld` doubles per row, the candidates at
// columns 0 .. M - 1, the reference points from column Mc on, zeros on the padding).  Two kernels per pick, no host round trip:
//
//   design_step_kernel  one pass over D: D[a, p] -= (piv[a] * piv[p]) * (1 / s) with the pick's row `piv`, and in the same pass
//                       the sums of w_p D[a, p]^2 over the columns of one chunk -> part[chunk][a].  Every element is read once
//                       and written once by ONE thread, the sums run in a fixed order: results repeat bit for bit.  Step 0 is
//                       this kernel with a zero pivot, so the score has one implementation.
//   design_pick_kernel  one workgroup: gain_a = (sum over the chunks in ascending order) / s_a, the argmax with the lowest index
//                       on a tie, the pick, its gain and 1 / s, and the snapshot of the pick's row for the next step.
//
// Kernel boundaries order everything: no workgroup waits on another, no atomics, vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covariance.hpp"
#include "design_plan.hpp"

namespace gmb {

typedef double design_d2 __attribute__((ext_vector_type(2)));

// the control block the two kernels share
enum : int { DESIGN_CTL_INV_S = 0, DESIGN_CTL_STOPPED = 1 };

struct DesignStepArgs {
  double* D;
  int64_t ld;         // doubles per row: a multiple of 128
  int64_t M;          // candidate rows
  int64_t Mc;         // stride of the partial sums
  const double* piv;  // the pick's row (ld), zero before the first pick
  const double* w;    // weights by column (ld): zero on the candidates and on the padding
  const double* ctl;  // [DESIGN_CTL_INV_S]
  double* part;       // [chunk][Mc]
};

// grid (chunks, ceil(M / DESIGN_ROWS)).  A thread owns four pairs of columns of its chunk, 512 columns apart, for each of the
// workgroup's rows; the pivot row's entries and the weights of those columns stay in registers over the rows.
__global__ __launch_bounds__(DESIGN_THREADS) void design_step_kernel(DesignStepArgs a) {
  __shared__ double red[DESIGN_ROWS][DESIGN_THREADS];
  constexpr int NP = DESIGN_CHUNK / (2 * DESIGN_THREADS);  // pairs per thread and row
  const int tid = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * DESIGN_CHUNK + 2 * tid;
  const int64_t a0 = (int64_t)blockIdx.y * DESIGN_ROWS;
  const double inv_s = a.ctl[DESIGN_CTL_INV_S];
  design_d2 pv[NP], wv[NP];
  bool in[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int64_t col = c0 + (int64_t)k * 2 * DESIGN_THREADS;
    in[k] = col < a.ld;  // (ld is even: a pair is inside or outside as a whole)
    pv[k] = in[k] ? *reinterpret_cast<const design_d2*>(a.piv + col) : design_d2{0.0, 0.0};
    wv[k] = in[k] ? *reinterpret_cast<const design_d2*>(a.w + col) : design_d2{0.0, 0.0};
  }
#pragma unroll
  for (int r = 0; r < DESIGN_ROWS; ++r) {
    const int64_t row = a0 + r;
    double acc = 0.0;
    if (row < a.M) {  // (block-uniform)
      const double pa = a.piv[row];
      double* drow = a.D + row * a.ld;
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        if (!in[k]) continue;
        design_d2* at = reinterpret_cast<design_d2*>(drow + c0 + (int64_t)k * 2 * DESIGN_THREADS);
        design_d2 d = *at;
        d.x -= (pa * pv[k].x) * inv_s;
        d.y -= (pa * pv[k].y) * inv_s;
        *at = d;
        acc = fma(wv[k].x, d.x * d.x, acc);
        acc = fma(wv[k].y, d.y * d.y, acc);
      }
    }
    red[r][tid] = acc;
  }
  __syncthreads();
  for (int s = DESIGN_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int r = 0; r < DESIGN_ROWS; ++r) red[r][tid] += red[r][tid + s];
    }
    __syncthreads();
  }
  if (tid < DESIGN_ROWS && a0 + tid < a.M) a.part[(int64_t)blockIdx.x * a.Mc + a0 + tid] = red[tid][0];
}

struct DesignPickArgs {
  const double* D;
  int64_t ld, M, Mc, nchunk;
  const double* part;
  const double* noise;  // M: what a prediction with noise adds to the candidate's variance (zeros without)
  int32_t* mask;        // M: 1 = not to be picked (again)
  double* ctl;
  double* piv;
  double* gains;    // q
  int64_t* picks;   // q
  double* score0;   // M, written at t == 0
  int32_t t;
  int32_t allow_repeats;
  int32_t score_only;  // q == 0: the scores and nothing else
};

// the better of two (gain, index) pairs: the larger gain, the lower index on a tie; index -1 = nobody
__device__ __forceinline__ void design_better(double& g, int64_t& i, const double g2, const int64_t i2) {
  if (i2 >= 0 && (i < 0 || g2 > g || (g2 == g && i2 < i))) g = g2, i = i2;
}

__global__ __launch_bounds__(DESIGN_PICK_THREADS) void design_pick_kernel(DesignPickArgs a) {
  __shared__ double bg[DESIGN_PICK_THREADS];
  __shared__ int64_t bi[DESIGN_PICK_THREADS];
  const int tid = threadIdx.x;
  if (a.ctl[DESIGN_CTL_STOPPED] != 0.0) {  // (uniform: written by an earlier launch only)
    if (tid == 0) a.picks[a.t] = -1, a.gains[a.t] = 0.0;
    return;
  }
  double g = 0.0;
  int64_t best = -1;
  for (int64_t c = tid; c < a.M; c += DESIGN_PICK_THREADS) {
    double sum = 0.0;
    for (int64_t k = 0; k < a.nchunk; ++k) sum += a.part[k * a.Mc + c];
    const double s = a.D[c * a.ld + c] + a.noise[c];
    const double gain = sum / s;
    const bool ok = s > 0.0 && s <= 1.79769313486231570815e308 && gain <= 1.79769313486231570815e308 && gain == gain && !a.mask[c];
    if (a.t == 0 && a.score0) a.score0[c] = ok ? gain : 0.0;
    if (ok && gain > 0.0 && (best < 0 || gain > g)) g = gain, best = c;  // (ascending c: the first of equals stays)
  }
  if (a.score_only) return;
  bg[tid] = g;
  bi[tid] = best;
  __syncthreads();
  for (int s = DESIGN_PICK_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      double g1 = bg[tid];
      int64_t i1 = bi[tid];
      design_better(g1, i1, bg[tid + s], bi[tid + s]);
      bg[tid] = g1;
      bi[tid] = i1;
    }
    __syncthreads();
  }
  const int64_t pick = bi[0];
  if (pick < 0) {  // nobody has a positive finite gain: this and every later pick is -1, the next step changes nothing
    if (tid == 0) {
      a.picks[a.t] = -1;
      a.gains[a.t] = 0.0;
      a.ctl[DESIGN_CTL_INV_S] = 0.0;
      a.ctl[DESIGN_CTL_STOPPED] = 1.0;
    }
    return;
  }
  if (tid == 0) {
    a.picks[a.t] = pick;
    a.gains[a.t] = bg[0];
    a.ctl[DESIGN_CTL_INV_S] = 1.0 / (a.D[pick * a.ld + pick] + a.noise[pick]);
    if (!a.allow_repeats) a.mask[pick] = 1;
  }
  const design_d2* src = reinterpret_cast<const design_d2*>(a.D + pick * a.ld);
  design_d2* dst = reinterpret_cast<design_d2*>(a.piv);
  for (int64_t p = tid; p < a.ld / 2; p += DESIGN_PICK_THREADS) dst[p] = src[p];
}

// what a prediction with noise adds to the variance of each candidate (kss_kernel's own term), zeros without
struct DesignNoiseArgs {
  CovParams p;  // the first pass's parameters
  PointSet pts;
  int32_t with_noise;
  double* noise;
};
__global__ void design_noise_kernel(DesignNoiseArgs a) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= a.pts.npad) return;
  a.noise[m] = (a.with_noise && m < a.pts.n) ? kss_noise(a.p, a.pts, m) : 0.0;
}

// out[0] = sum_p w[p] var[p] over the ld columns, in a fixed order (one workgroup)
__global__ __launch_bounds__(DESIGN_PICK_THREADS) void design_ivar_kernel(const double* w, const double* var, int64_t ld, double* out) {
  __shared__ double red[DESIGN_PICK_THREADS];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int64_t p = tid; p < ld; p += DESIGN_PICK_THREADS) acc = fma(w[p], var[p], acc);
  red[tid] = acc;
  __syncthreads();
  for (int s = DESIGN_PICK_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) out[0] = red[0];
}

}  // namespace gmb
