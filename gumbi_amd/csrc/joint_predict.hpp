// joint_predict.hpp -- the JOINT posterior at M test points: full covariance and correlated draws.
//
// pm.gp.Marginal.conditional(..., diag=False) (gumbi/regression/pymc/GP.py:914-917, draw_point_samples / draw_grid_samples)
// needs, beyond gmb_predict's mean and diagonal,
//
//   C  = K(X*, X*) - V V^T (+ noise) + jitter I        V = K(X*, X) L^-T, all M rows at once (m fastest, as gmb_predict's dV)
//   L* = chol(C)                                       the engine's own leaf / strip / tile kernels on a SECOND matrix
//   Y  = 1 mu^T + Z L*^T                               S draws from caller-supplied standard normals
//
// The covariance build (cov_tile_kernel, COV_TRAIN on the test points), the rank-N update (gemm_f64, tri) and the
// factorisation are the training path's kernels; the host side that strings them over the second matrix is in engine.hip
// (joint_*).  This header holds the second matrix's state and the two kernels particular to the path:
//
//   joint_draw_kernel        Y^T = mu 1^T + L* Z^T: a skinny f64-MFMA product with a lower-triangular operand, the mean and the
//                            transpose into numpy's S x M row-major layout fused into its epilogue
//   joint_symmetrise_kernel  both triangles of the row-major M x M covariance from the lower-triangle tiles
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_buffers.hpp"
#include "gemm_f64.hpp"

namespace gmb {

// Everything the factorisation of C owns (the blocks belong to the engine's pool: device_buffers.hpp).  The host routines of the Cholesky (chol_factor, chol_tiles, chol_cols, ...) are told
// the matrix they work on -- its 16 x 16 diagonal inverses, scalar block, info word and tile-kernel control block with it
// (engine.hip: FactorRef, joint_factor_ref) -- so nothing of the training factorisation -- its factor, log-determinant, failure
// index, control words -- is written by a draw.
struct JointState {
  int64_t M = 0, Mp = 0, Mr = 0;  // test points; padded to 128; rows of the bordered layout the Cholesky kernels expect ((M + 1) up)
  DevBuf<double> dC;              // Mr x Mp column-major, leading dimension Mr: lower-triangle tiles of C, then of L*
  DevBuf<double> dDinv16;         // 8 x (16 x 16) sub-block inverses per diagonal block
  DevBuf<double> dscal;           // head of the engine's scalar-block layout: [0] log-det of C, [64] the info word (int32)
  DevBuf<uint32_t> dct;           // control block of the persistent tile kernel
  DevBuf<double> dzero;           // Mp zeros: the bordered layout's extra row (the training build puts y there)
  DevBuf<double> dstage;          // device staging of host-side cov / Z / Y
};

// ---- the draw ---------------------------------------------------------------------------------------------------------------
struct DrawArgs {
  const double* L;     // L*(m, j) at L + m + j * ldl, lower triangle (whatever lies above the diagonal is never used)
  int64_t ldl;
  const double* Z;     // Z(s, j) at Z + s * ldz + j
  int64_t ldz;
  const double* mean;  // M, or nullptr (no shift)
  double* Y;           // Y(s, m) at Y + s * ldy + m
  int64_t ldy;
  int64_t M;
  int32_t S;
};

// Y(s, m) = mean(m) + sum_{j <= m} L*(m, j) Z(s, j).
//
// Tile shape (skinny: S is 1 .. 1000 against M ~ 10^4, so the product is bound by the one pass over L*'s M^2 / 2 doubles, not by
// the matrix pipe): a workgroup owns 16 rows of L* x 16 NS draws; its four waves split the CONTRACTION, wave w taking the
// k-quads 4 w, 4 w + 16, ... up to the row block's last column (the triangular operand: nothing right of the diagonal is read),
// each as one v_mfma_f64_16x16x4_f64 per 16 draws with L* as the m operand (16 consecutive rows of a column: 128 B lines) and Z
// as the n operand.  16-row blocks give M / 16 workgroups (625 at M = 10^4: 2.4 per compute unit, longest contraction
// dispatched first) where 128-row tiles would leave two thirds of the chip idle.  The four partial tiles meet in LDS and are
// added in wave order -- the same bits run to run -- with the mean, and leave as rows of Y: the MFMA's D layout has m along the
// registers, LDS turns it so that 16 consecutive m of one draw are written as one 128 B line.
template <int NS>
__global__ __launch_bounds__(256) void joint_draw_kernel(DrawArgs a) {
  __shared__ double red[4][16 * NS][17];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const int64_t r0 = (int64_t)(gridDim.x - 1 - blockIdx.x) * 16;  // longest contractions first
  const int s0 = (int)blockIdx.y * 16 * NS;
  const int64_t row = r0 + r16;
  const bool row_ok = row < a.M;
  const int64_t kend = r0 + 16 < a.M ? r0 + 16 : a.M;

  d4 acc[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
  const double* zrow[NS];
  bool s_ok[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) {
    const int s = s0 + q * 16 + r16;
    s_ok[q] = s < a.S;
    zrow[q] = a.Z + (int64_t)(s_ok[q] ? s : 0) * a.ldz;
  }
  for (int64_t k0 = 4 * wave; k0 < kend; k0 += 16) {
    const int64_t j = k0 + kq;
    const double av = (row_ok && j <= row) ? a.L[row + j * a.ldl] : 0.0;  // (j <= row < M: inside the matrix)
    const bool j_ok = j < a.M;
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      const double bv = (s_ok[q] && j_ok) ? zrow[q][j] : 0.0;
      acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[q], 0, 0, 0);
    }
  }
  // D layout: n (draw) = lane & 15, m (row of L*) = (lane >> 4) + 4 * reg
#pragma unroll
  for (int q = 0; q < NS; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][q * 16 + r16][kq + 4 * r] = acc[q][r];
  __syncthreads();
  for (int idx = tid; idx < 256 * NS; idx += 256) {
    const int sl = idx >> 4, ml = idx & 15;
    const int s = s0 + sl;
    const int64_t m = r0 + ml;
    if (s < a.S && m < a.M) {
      const double dot = ((red[0][sl][ml] + red[1][sl][ml]) + red[2][sl][ml]) + red[3][sl][ml];
      a.Y[(int64_t)s * a.ldy + m] = a.mean ? a.mean[m] + dot : dot;
    }
  }
}

// ---- symmetrise on output ---------------------------------------------------------------------------------------------------
struct SymArgs {
  const double* C;  // C(i, j), i >= j, at C + i + j * ldc
  int64_t ldc;
  double* out;      // out[i * ldo + j], both triangles
  int64_t ldo;
  int64_t M;
};

// grid (nb, nb), nb = ceil(M / 32); block (bi, bj) with bj <= bi copies the 32 x 32 block (bi, bj) of the lower triangle to
// out's block (bi, bj) -- transposed through LDS, the row-major output's fast index is the source's slow one -- and to its
// mirror image (bj, bi), which has the source's own orientation.  A diagonal block is completed from its lower half first.
__global__ __launch_bounds__(256) void joint_symmetrise_kernel(SymArgs a) {
  __shared__ double tile[32][33];  // tile[j][i] = C(i0 + i, j0 + j)
  const int bi = blockIdx.x, bj = blockIdx.y;
  if (bj > bi) return;
  const int64_t i0 = (int64_t)bi * 32, j0 = (int64_t)bj * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int j = ty; j < 32; j += 8) {
    const int64_t i = i0 + tx, jj = j0 + j;
    tile[j][tx] = (i < a.M && jj < a.M && i >= jj) ? a.C[i + jj * a.ldc] : 0.0;
  }
  __syncthreads();
  const bool diag = bi == bj;
  // value of C(i0 + il, j0 + jl) by symmetry
  auto val = [&](int il, int jl) { return (diag && il < jl) ? tile[il][jl] : tile[jl][il]; };
  for (int j = ty; j < 32; j += 8) {  // mirror block: out(j0 + j, i0 + tx), i fastest
    const int64_t i = i0 + tx, jj = j0 + j;
    if (i < a.M && jj < a.M) a.out[jj * a.ldo + i] = val(tx, j);
  }
  if (diag) return;
  for (int r = ty; r < 32; r += 8) {  // the block itself: out(i0 + r, j0 + tx), j fastest
    const int64_t i = i0 + r, jj = j0 + tx;
    if (i < a.M && jj < a.M) a.out[i * a.ldo + jj] = val(r, tx);
  }
}

}  // namespace gmb
