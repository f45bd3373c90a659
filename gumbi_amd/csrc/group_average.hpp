// group_average.hpp -- averages of the posterior over GROUPS of points: marginal effects and contrasts.
//
// For groups g of points x_m with weights w_m (any sign), fbar_g = sum_{m in g} w_m f(x_m) is Gaussian with
//
//   a_g   = sum_{m in g} w_m k(x_m, X)                               row g of A (G x N)
//   Q_gh  = sum_{m in g} sum_{m' in h} w_m w_m' k(x_m, x_m')          G x G
//   V_A   = A L^-T            mean = V_A v            cov = Q - V_A V_A^T            (v = L^-1 y)
//
// -- the joint posterior with G right-hand sides in place of M, and nothing of size M x M or M x N anywhere.  Once A sits where a
// prediction keeps its cross-covariance (dV, group index fastest) and Q where the joint posterior keeps K(X*, X*) (the second
// matrix), the rest IS gmb_predict / gmb_predict_joint: predict_solve_v, predict_reduce and the rank-N update (engine.hip).
// This header holds the kernels that form A and Q without writing a covariance row:
//
//   group_cov_partial_kernel<KIND, NC, GEN>   part[task][column] = sum_{m in task} w_m k(x_m, column point): a workgroup = 64
//       column points (one per lane, coordinates in registers) x 4 waves; blockIdx.y names a TASK, a run of at most GROUP_CHUNK
//       consecutive points of one group (group_tasks.hpp), staged through LDS in pieces of which every wave takes a quarter --
//       the shape of predict_grad_partial_kernel.  The pair value is cov_general_tile's one expression: eta^2 f(r^2) from direct
//       scaled differences on the prepared columns (periodic models need nothing extra), for GEN + tau <xl, xl'>, times the
//       coregion table entries.  One accumulator per lane; the four waves' sums meet in LDS and are added in the order 0 + 1 + 2 + 3.
//   group_cov_finish_kernel                    out[g + column ldo] = the group's task partials added in ascending task order: a
//       store for the first selected term, an add for an additive model's further terms.
//   group_fold_kernel                          Q[g, h] = sum_{m' in h} w_m' R[g, m'], h <= g, in ascending m', into the second
//       matrix's bordered layout, the diagonal also into kss.
//
// The same pair serves both reductions.  A: columns = the training points, out = dV (leading dimension Gr).  Q: columns = the
// group points themselves, out = R (128 groups x M, group index fastest), one row block of 128 groups at a time, folded at once.
// A caller that wants no covariance needs Q's diagonal only: a task's column blocks outside its own group's point range then
// return at once (a block-uniform test), sum |g|^2 pairs instead of M^2, and the finish and the fold touch that range only.
//
// No atomics, and no workgroup waits for another -- plain launches in stream order -- so the same bits call after call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covariance.hpp"
#include "group_tasks.hpp"
#include "workspace_sizes.hpp"  // GA_ROWS

namespace gmb {

constexpr int GA_COLS = 64;     // column points per workgroup (a lane each)
constexpr int GA_PIECE = 128;   // group points staged in LDS at a time
static_assert(GROUP_CHUNK % GA_PIECE == 0, "a task is a whole number of staged pieces at most");

struct GroupCovArgs {
  CovParams p;
  PointSet pts;            // the group points, prepared (all M of the call)
  PointSet cols;           // the column points
  const double* w;         // weight per group point
  const int64_t* tasks;    // (group, first point, count) of the launch's task 0 (blockIdx.y = 0) and on
  double* part;            // part[blockIdx.y * ldp + column]
  int64_t ldp;             // columns the grid covers: a multiple of 64, <= cols.npad
  const int64_t* offsets;  // diag_only: the groups' point ranges
  int32_t diag_only;       // columns are the group points; only the task's own group's columns are wanted
};

template <int KIND, int NC, bool GEN>
__global__ __launch_bounds__(256) void group_cov_partial_kernel(GroupCovArgs a) {
  constexpr int NCS = (NC + 2) & ~1;  // row stride of the staged points: NC coordinates, the weight, padded to even
  constexpr int NL = GEN ? MAX_LIN : 0;
  constexpr int STAGE = GA_PIECE * NCS + GA_PIECE * NL + (GEN ? GA_PIECE * MAX_TABS / 2 : 0);  // doubles
  constexpr int RED = 3 * GA_COLS;
  __shared__ double smem[STAGE > RED ? STAGE : RED];
  double* sx = smem;                                                       // [GA_PIECE][NCS]
  double* sl = smem + GA_PIECE * NCS;                                      // [GA_PIECE][MAX_LIN]
  int32_t* sc = reinterpret_cast<int32_t*>(smem + GA_PIECE * (NCS + NL));  // [GA_PIECE][MAX_TABS]: table offset + row of the entry
  (void)sl;
  (void)sc;
  const CovParams& p = a.p;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t* task = a.tasks + 3 * (int64_t)blockIdx.y;
  const int64_t m0 = task[1], m1 = m0 + task[2];  // within [0, pts.n): the host built the list from checked offsets
  const int64_t c0 = (int64_t)blockIdx.x * GA_COLS;
  if (a.diag_only) {  // (block-uniform, before any barrier)
    const int64_t lo = a.offsets[task[0]], hi = a.offsets[task[0] + 1];
    if (c0 + GA_COLS <= lo || c0 >= hi) return;
  }
  const int64_t c = c0 + lane;  // < ldp <= cols.npad: the grid covers ldp / 64 blocks exactly

  double xi[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) xi[k] = a.cols.xs[(int64_t)k * a.cols.npad + c];
  double li[NL > 0 ? NL : 1];
  int ci[MAX_TABS];
  (void)li;
  (void)ci;
  if constexpr (GEN) {
#pragma unroll
    for (int l = 0; l < NL; ++l) li[l] = l < p.n_lin ? a.cols.xl[(int64_t)l * a.cols.npad + c] : 0.0;
#pragma unroll
    for (int t = 0; t < MAX_TABS; ++t) ci[t] = t < p.n_tab ? a.cols.cat[(int64_t)t * a.cols.npad + c] : 0;
  }
  double acc = 0.0;

  for (int64_t q0 = m0; q0 < m1; q0 += GA_PIECE) {
    const int cnt = (int)(m1 - q0 < GA_PIECE ? m1 - q0 : GA_PIECE);
    __syncthreads();  // the previous piece has been read
    for (int idx = tid; idx < (NC + 1) * GA_PIECE; idx += 256) {
      const int k = idx / GA_PIECE, j = idx - k * GA_PIECE;
      if (j < cnt) sx[j * NCS + k] = k < NC ? a.pts.xs[(int64_t)k * a.pts.npad + q0 + j] : a.w[q0 + j];
    }
    if constexpr (GEN) {
      for (int idx = tid; idx < p.n_lin * GA_PIECE; idx += 256) {
        const int k = idx / GA_PIECE, j = idx - k * GA_PIECE;
        if (j < cnt) sl[j * MAX_LIN + k] = a.pts.xl[(int64_t)k * a.pts.npad + q0 + j];
      }
      for (int idx = tid; idx < p.n_tab * GA_PIECE; idx += 256) {
        const int t = idx / GA_PIECE, j = idx - t * GA_PIECE;
        if (j < cnt) sc[j * MAX_TABS + t] = p.tab_off[t] + a.pts.cat[(int64_t)t * a.pts.npad + q0 + j] * p.tab_levels[t];
      }
    }
    __syncthreads();
    const int j_lo = wave * (GA_PIECE / 4);
    const int j_hi = j_lo + GA_PIECE / 4 < cnt ? j_lo + GA_PIECE / 4 : cnt;
#pragma unroll 2
    for (int j = j_lo; j < j_hi; ++j) {
      const double* row = sx + j * NCS;
      double r2 = 0.0;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const double d = row[k] - xi[k];
        r2 = fma(d, d, r2);
      }
      double v = p.eta2 * stationary<KIND>(r2);
      if constexpr (GEN) {
        if (p.n_lin > 0) {
          double s = 0.0;
#pragma unroll
          for (int l = 0; l < NL; ++l)
            if (l < p.n_lin) s = fma(sl[j * MAX_LIN + l], li[l], s);
          v = fma(p.tau, s, v);
        }
#pragma unroll
        for (int t = 0; t < MAX_TABS; ++t)
          if (t < p.n_tab) v *= p.tabs[sc[j * MAX_TABS + t] + ci[t]];
      }
      acc = fma(row[NC], v, acc);
    }
  }

  // waves 1 .. 3 hand their sums to wave 0, which adds them in wave order and writes the task's partial
  double* red = smem;  // [3][GA_COLS]
  __syncthreads();     // the staging area is free
  if (wave > 0) red[(wave - 1) * GA_COLS + lane] = acc;
  __syncthreads();
  if (wave == 0) {
    double v = acc;
#pragma unroll
    for (int w = 0; w < 3; ++w) v += red[w * GA_COLS + lane];
    a.part[(int64_t)blockIdx.y * a.ldp + c] = c < a.cols.n ? v : 0.0;  // columns of no point are zero
  }
}

struct GroupFinishArgs {
  const double* part;
  int64_t ldp;
  const int64_t* first_task;  // group g's tasks: first_task[g] .. first_task[g + 1] - 1 (indices into the call's whole list)
  int64_t task0;              // the task whose partials are row 0 of `part`
  int64_t g0, ng;             // the groups of this pass
  int64_t ncols;              // columns written (<= ldp)
  double* out;                // out[(g - g0) + column * ldo]
  int64_t ldo;
  int32_t accumulate;
  const int64_t* offsets;     // diag_only: only the columns of the group's own points exist in `part`, and only they are written
  int32_t diag_only;
};

// grid: ng x ceil(ncols / 256) workgroups along x, a group's column blocks next to each other; a thread per column
__global__ __launch_bounds__(256) void group_cov_finish_kernel(GroupFinishArgs a) {
  const int64_t ncb = (a.ncols + 255) / 256;
  const int64_t gl = (int64_t)blockIdx.x / ncb, cb = (int64_t)blockIdx.x - gl * ncb;
  const int64_t c = cb * 256 + threadIdx.x;
  if (gl >= a.ng || c >= a.ncols) return;
  const int64_t g = a.g0 + gl;
  if (a.diag_only && (c < a.offsets[g] || c >= a.offsets[g + 1])) return;
  double s = 0.0;
  for (int64_t t = a.first_task[g]; t < a.first_task[g + 1]; ++t) s += a.part[(t - a.task0) * a.ldp + c];
  double* o = a.out + gl + c * a.ldo;
  *o = a.accumulate ? *o + s : s;
}

struct GroupFoldArgs {
  const double* R;         // R[(g - g0) + GA_ROWS * m']
  const double* w;
  const int64_t* offsets;
  int64_t g0, G;
  double* C;               // Q(g, h), h <= g, at C + g + h * ldc; null: the diagonal only
  int64_t ldc;
  double* kss;             // Q(g, g)
  int32_t accumulate;
  int32_t diag_only;       // h = g only (grid of one workgroup)
};

// grid: a workgroup per column group h = 0 .. min(G, g0 + 128) - 1, thread = row group of the block
__global__ __launch_bounds__(GA_ROWS) void group_fold_kernel(GroupFoldArgs a) {
  const int gl = threadIdx.x;
  const int64_t g = a.g0 + gl;
  if (g >= a.G) return;
  const int64_t h = a.diag_only ? g : (int64_t)blockIdx.x;
  if (h > g) return;
  double s = 0.0;
  const double* r = a.R + gl;
  for (int64_t m = a.offsets[h]; m < a.offsets[h + 1]; ++m) s = fma(a.w[m], r[m * GA_ROWS], s);
  if (a.C) {
    double* o = a.C + g + h * a.ldc;
    *o = a.accumulate ? *o + s : s;
  }
  if (h == g) a.kss[g] = a.accumulate ? a.kss[g] + s : s;
}

// the variance of the reduction on the diagonal of the row-major covariance: cov's diagonal IS var, to the bit
__global__ __launch_bounds__(256) void group_cov_diag_kernel(double* out, int64_t ldo, int64_t G, const double* var) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g < G) out[g * ldo + g] = var[g];
}

}  // namespace gmb
