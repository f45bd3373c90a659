// gemm_splitk.hpp -- the dense contraction of gemm_f64.hpp for FEW output tiles and a LONG contraction, split along k.
//
//   C[n + m*ldc] = beta * C[n + m*ldc] + alpha * sum_{k < K} A[m + k*lda] * B[n + k*ldb]
//
// (column-major, both operands k-major, m and n multiples of 128, K of 16; tri: tiles strictly above the diagonal, tn < tm,
// are left alone).  gemm_f64.hpp gives every 128 x 128 output tile to ONE workgroup: right for the trailing updates, whose
// launches have thousands of tiles, wrong for the corner update of gmb_append -- one to a handful of tiles contracted over
// every kept column of the factor (N = 50k, one tile: 1.6 GF on one compute unit while 255 idle).  Here the work of a tile is
// cut into S slices of the contraction, in two launches in stream order:
//   1. gemm_f64_splitk_partial_kernel, grid (S, tiles): workgroup (s, t) contracts k in [s*len, min(K, (s+1)*len)) of tile t with
//      gemm_f64_body (its staging, its MFMA loop, its epilogue with alpha = 1, beta = 0) and writes the 128 x 128 partial to the
//      workspace ws[t][s][128*128];
//   2. gemm_f64_splitk_reduce_kernel: every element of every computed tile adds its S partials in ASCENDING slice order and
//      applies alpha and beta to C.
// No atomics, no arrival counters, no workgroup waits for another; every partial and every element of C is written once, the
// sums have one order: the same bits call after call.  S is a function of (tile count, K) alone (splitk_rule), never of the
// device's state.  S = 1 is the degenerate shape's path (one slice, the reduction copies it through alpha / beta).
#pragma once
#include "gemm_f64.hpp"
#include "append_layout.hpp"

namespace gmb {

struct SplitKArgs {
  double* C;
  int64_t ldc;
  const double* A;
  int64_t lda;
  const double* B;
  int64_t ldb;
  int32_t mt, nt;     // 128-tiles along m and n
  int32_t k;          // multiple of KT
  int32_t tri;        // skip tiles with tn < tm
  int32_t slices;     // S
  int32_t slice_len;  // k extent of a slice (multiple of KT); the last slice may be shorter, never empty
  double alpha, beta;
  double* ws;         // [tile][slice][TILE * TILE]
};

__global__ __launch_bounds__(256, 2) void gemm_f64_splitk_partial_kernel(SplitKArgs a) {
  const int s = blockIdx.x, t = blockIdx.y;
  int tm, tn;
  splitk_decode_tile(t, a.nt, a.tri, tm, tn);
  const int64_t k0 = (int64_t)s * a.slice_len;
  const int64_t kn = a.k - k0 < a.slice_len ? a.k - k0 : a.slice_len;
  if (kn <= 0) return;  // (never: the host refuses empty slices)
  // the slice as a one-tile product of its own
  GemmArgs g{};
  g.C = a.ws + ((int64_t)t * a.slices + s) * (TILE * TILE);
  g.ldc = TILE;
  g.A = a.A + (int64_t)tm * TILE + k0 * a.lda;
  g.lda = a.lda;
  g.B = a.B + (int64_t)tn * TILE + k0 * a.ldb;
  g.ldb = a.ldb;
  g.mt = g.nt = 1;
  g.k = (int32_t)kn;
  g.alpha = 1.0;
  g.beta = 0.0;
  g.nblk_stride = 1;
  g.order = 1;  // block 0 = tile (0, 0) of the n-major list
  gemm_f64_body<2, 2, 4, 4>(g, 0);
}

// grid (TILE * TILE / 256, tiles): one element per thread, partials read along the contiguous index
__global__ __launch_bounds__(256) void gemm_f64_splitk_reduce_kernel(SplitKArgs a) {
  const int t = blockIdx.y;
  int tm, tn;
  splitk_decode_tile(t, a.nt, a.tri, tm, tn);
  const int idx = blockIdx.x * 256 + threadIdx.x;  // n + m * TILE inside the tile
  const int mm = idx >> 7, nn = idx & (TILE - 1);
  const double* p = a.ws + (int64_t)t * a.slices * (TILE * TILE) + idx;
  double sum = p[0];
  for (int s = 1; s < a.slices; ++s) sum += p[(int64_t)s * (TILE * TILE)];
  double* c = a.C + (int64_t)tn * TILE + nn + ((int64_t)tm * TILE + mm) * a.ldc;
  if (a.beta == 0.0) *c = a.alpha * sum;
  else *c = a.beta * *c + a.alpha * sum;
}

}  // namespace gmb
