/*
 * gumbi_hip.h -- C ABI of libgumbi_hip.so, the MI355X (gfx950) exact-GP engine behind
 * Gumbi's `GP.fit() / prepare_grid() / predict_grid()`.
 *
 * The reference (JohnGoertz/Gumbi v0.4.1) has no FFI: its backend seam is the Python ABC
 * `gumbi.regression.base.Regressor` (gumbi/regression/base.py:21) whose subclasses implement
 * `fit` (:119-127), `build_model` (:129-137), `predict(points_array, with_noise) -> (mean, var)`
 * (:477-495) and `find_MAP` (called from :1064).  The arithmetic those methods reach lives in
 * PyMC (`pm.gp.Marginal`, `pm.gp.cov.*`, `pm.find_MAP`; call sites
 * gumbi/regression/pymc/GP.py:407-410, 453, 460-462, 560-561, 580, 811, 845-847).  Each entry
 * point below names the reference call it replaces.  INTEGRATION.md shows the ctypes stub a
 * Gumbi maintainer would add.
 *
 * Conventions
 *   - every function returns 0 (GMB_OK) or a negative gmb_status; nothing throws across the ABI;
 *   - a handle is NOT thread-safe, distinct handles are independent;
 *   - all matrices handed in are row-major float64 unless stated; all sizes are int64_t;
 *   - `memspace` says whether caller pointers are host (GMB_HOST) or device (GMB_DEVICE)
 *     memory; the library never retains a caller pointer after the call returns;
 *   - no torch / pybind types anywhere in the signatures.
 *
 * Parameter vector `theta` (natural scale), n = gmb_theta_size(spec):
 *   [ ls (n_cont if ard else 1) | eta | sigma |
 *     c (n_lin), tau                       -- only if n_lin > 0          (pymc/GP.py:451-453)
 *     per coregion dim: W (L x 2 row-major), kappa (L)                   (pymc/GP.py:459-462)
 *     W_out (P x 2), kappa_out (P)         -- only if out_col >= 0       (pymc/GP.py:724-727)
 *     W_noise (P x 2), kappa_noise (P)     -- only if out_col >= 0 && hetero_noise (:565-569) ]
 */
#ifndef GUMBI_HIP_H
#define GUMBI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMB_ABI_VERSION 16
#define GMB_MAX_DIMS 16   /* continuous dims per kernel */
#define GMB_MAX_LIN 8     /* linear dims per kernel (subset of the continuous dims) */
#define GMB_MAX_COREG 4   /* categorical (coregion) dims besides the output column */
#define GMB_MAX_LEVELS 32 /* levels per coregion table */

typedef enum gmb_status {
  GMB_OK = 0,
  GMB_EINVAL = -1,   /* bad argument / call order            (ValueError in Python)            */
  GMB_ENOMEM = -2,   /* hipMalloc failed                                                       */
  GMB_EHIP = -3,     /* a HIP runtime call or kernel launch failed; see gmb_last_error         */
  GMB_ENOTPD = -4,   /* covariance not positive definite; see gmb_notpd_index (LinAlgError)    */
  GMB_ENODEVICE = -5,/* no usable gfx950 device -- there is NO CPU fallback                    */
  GMB_ENOCONV = -6   /* gmb_laplace_evaluate: the Newton iteration hit one of its caps          */
} gmb_status;

typedef enum gmb_kernel_kind { /* pm.gp.cov.<name>, selected at pymc/GP.py:664-674,684 */
  GMB_EXPQUAD = 0,
  GMB_MATERN52 = 1,
  GMB_MATERN32 = 2,
  GMB_MATERN12 = 3,
  GMB_EXPONENTIAL = 4
} gmb_kernel_kind;

typedef enum gmb_memspace { GMB_HOST = 0, GMB_DEVICE = 1 } gmb_memspace;

/* Kernel structure Gumbi declares in PymcGP._construct_kernels (pymc/GP.py:652-757, non-additive):
 *   K = (eta^2 k_cont [+ tau Linear(c)]) * prod_dims Coregion_dim * Coregion_out
 *   noise = WhiteNoise(sigma) [* Coregion("Output_noise")]     (pymc/GP.py:560-569)
 *   Sigma = K + noise + jitter I                               (pm.gp.Marginal, jitter 1e-6) */
typedef struct gmb_kernel_spec {
  int32_t kind;                      /* gmb_kernel_kind                                        */
  int32_t ard;                       /* 1: one lengthscale per continuous dim (fit(ARD=True))  */
  int32_t n_cont;                    /* number of continuous dims (active_dims of k_cont)      */
  int32_t idx_cont[GMB_MAX_DIMS];    /* their column indices in X                              */
  int32_t n_lin;                     /* linear dims (subset of continuous)                     */
  int32_t idx_lin[GMB_MAX_LIN];
  int32_t n_coreg;                   /* categorical dims other than the output column          */
  int32_t coreg_col[GMB_MAX_COREG];
  int32_t coreg_levels[GMB_MAX_COREG];
  int32_t out_col;                   /* output-coregion column or -1 (single output)           */
  int32_t n_out;                     /* number of outputs P                                    */
  int32_t hetero_noise;              /* heteroskedastic_outputs (pymc/GP.py:565)               */
  int32_t additive;                  /* specify_model(additive=True) (pymc/GP.py:732-754): a global
                                      * kernel plus one kernel per coregion dim, each times that dim's
                                      * table (and the output table); theta gains, after the layout
                                      * above, one block [ls | eta | (c, tau)] per coregion dim     */
  double jitter;                     /* 1e-6 to follow pm.gp.Marginal                          */
} gmb_kernel_spec;

typedef struct gmb_timings { /* milliseconds on the engine's HIP stream (hipEvent pairs); see gmb_evaluate for when they are taken */
  double kbuild_ms;          /* covariance-matrix construction (last gmb_factorize)            */
  double chol_ms;            /* whole Cholesky (leaves + trsm + trailing updates)              */
  double chol_gemm_ms;       /* sum over the MFMA SYRK/GEMM trailing-update launches           */
  double chol_gemm_flops;    /* flops those launches performed (2*m*n*k per computed tile)     */
  int64_t chol_gemm_launches;
  double chol_leaf_ms;       /* diagonal-block potrf + triangular-inverse leaves               */
  double chol_trsm_ms;       /* panel solves                                                   */
  double predict_ms;         /* last gmb_predict, all tiles                                    */
  double predict_gemm_ms;
  double predict_gemm_flops;
  int64_t predict_gemm_launches;
  double grad_ms;            /* last gmb_nlml gradient (inverse + trace reductions)            */
  double grad_gemm_ms;
  double grad_gemm_flops;
  double kbuild_bytes;       /* algorithmic bytes the K-build wrote+read (8N(N+1)/2 + 8N(d+1)) */
  /* cumulative since the last gmb_set_profiling(e, 1): every MFMA GEMM launch of every phase */
  double total_gemm_ms;
  double total_gemm_flops;
  int64_t total_gemm_launches;
  double total_kbuild_ms;
  double total_kbuild_bytes;
  int64_t total_kbuild_launches;
  /* the part of total_gemm_* that ran on the CU-masked bulk stream (trailing updates of the masked
     look-ahead schedule: masked_cus of the device's compute units were available to them)        */
  double masked_gemm_ms;
  double masked_gemm_flops;
  int64_t masked_cus;
  /* wall time with at least one GEMM launch in flight (union of the launch intervals: launches of
     the look-ahead schedules' two streams overlap, total_gemm_ms is the SUM of their durations)    */
  double total_gemm_wall_ms;
  /* the Cholesky's BULK trailing-update launches alone (U1 / U2 of the look-ahead schedules, every update
     of the plain recursion, the UPDATE steps of the multi-GPU driver), cumulative like total_gemm_*: the
     kernel launches the north star's MFMA-utilisation target is stated on.  The small in-panel products
     of the latency-bound panel chain are counted separately (total_chol_panel_gemm_*).               */
  double total_chol_gemm_ms;
  double total_chol_gemm_flops;
  int64_t total_chol_gemm_launches;
  double total_chol_gemm_wall_ms; /* union of their launch intervals */
  double total_chol_panel_gemm_ms;
  double total_chol_panel_gemm_flops;
  /* multi-GPU driver (gmb_dist_*), this rank, HIP events around every collective and at every stream join.
     chol_*: the last gmb_dist_factorize; grad_*: the last gmb_dist_nlml with a gradient.
       comm_ms         sum over the all-gathers of (stream reached the collective -> collective complete):
                       transfer time plus the wait for the slowest peer
       comm_exposed_ms the part of comm_ms that nothing hid.  Factorisation: per panel, min(time the bulk
                       stream sat idle waiting for the panel chain, time that chain spent in its two
                       all-gathers) -- the first chain has nothing to hide behind and counts in full.
                       Gradient: the main stream's wait for the communication stream after the last chunk
                       plus the two small all-gathers (alpha, accumulators) that sit on the main stream
       main_wait_ms    main stream waiting for the bulk stream at the JOINs (trailing update U2 longer than
                       the next panel's chain: communication fully hidden there)
       bulk_wait_ms    bulk stream waiting for the main stream at the FORKs (chain-bound time)          */
  int64_t dist_world;             /* ranks of the communicator the last gmb_dist_* call ran on            */
  int64_t dist_chol_collectives;
  double dist_chol_comm_bytes;    /* bytes received from the other ranks                                  */
  double dist_chol_comm_ms;
  double dist_chol_comm_exposed_ms;
  double dist_chol_main_wait_ms;
  double dist_chol_bulk_wait_ms;
  int64_t dist_grad_collectives;
  double dist_grad_comm_bytes;
  double dist_grad_comm_ms;
  double dist_grad_comm_exposed_ms;
  /* Every rank computes the factorisation's failure index, log-determinant and |v|^2 redundantly (bit-identical by
     construction); all ranks nevertheless LEAVE gmb_dist_factorize with rank 0's copy, so that optimisers running in
     lock step on every rank can never part company.  Cumulative count of ranks whose own copy differed (expected 0). */
  int64_t dist_lockstep_repairs;
  /* The persistent tile Cholesky (csrc/chol_tiles.hpp: the WHOLE factorisation of a small matrix -- contraction, leaves and
     strip solves -- in one launch), cumulative like total_gemm_*: launch durations (HIP events), the flops of the tiles'
     contractions, launches.  Such a factorisation has no separate trailing-update launches: total_chol_gemm_* stay 0. */
  double total_chol_tile_ms;
  double total_chol_tile_flops;
  int64_t total_chol_tile_launches;
  /* The persistent evaluation launch (csrc/eval_tiles.hpp: L^-T by rows and Sigma^-1 = U U^T as tile tasks -- in gmb_evaluate
     together with the factorisation's own tile tasks, ONE launch for the matrix work of a MAP evaluation), cumulative:
     launch durations, contraction flops (factorisation included when it rode along), launches. */
  double total_eval_tile_ms;
  double total_eval_tile_flops;
  int64_t total_eval_tile_launches;
  /* (ABI 10) every launch the Cholesky's schedules issue AS a trailing update, whatever tile shape it runs -- the population
     `total_chol_gemm_*` covered up to round 4; since round 5 total_chol_gemm_* holds only the updates large enough for the
     128 x 128 kernel (gemm_f64_dma_chol_update_kernel).  Cumulative like total_gemm_*. */
  double total_chol_update_all_ms;
  double total_chol_update_all_flops;
  int64_t total_chol_update_all_launches;
  /* (ABI 10) 1 when the last gmb_predict formed A^T = K(X*, X) L^-T as one GEMM against the inverse factor the fit's last
     gradient evaluation left behind (csrc/predict_form.hpp), 0 when it solved against L (gmb_set_predict_form) */
  int64_t predict_gemm_form;
  /* (ABI 10) the bottom panels of the large matrices' recursion as launches of the tile kernel (csrc/engine.hip:
     chol_tiles_panel): durations, contraction flops, launches -- a subset of total_chol_panel_gemm_* */
  double total_chol_panel_tile_ms;
  double total_chol_panel_tile_flops;
  int64_t total_chol_panel_tile_launches;
} gmb_timings;

typedef struct gmb_engine gmb_engine;

/* -- lifecycle ------------------------------------------------------------------------------ */

/* Number of visible HIP devices, or a negative gmb_status.  Never falls back to the CPU. */
int gmb_device_count(void);
int gmb_abi_version(void);

/* Create an engine bound to HIP device `device`.  `stream` is an existing hipStream_t to launch
 * on (e.g. torch's current stream), or NULL to let the engine create its own. */
int gmb_create(gmb_engine** out, int32_t device, void* stream);
/* A second engine on `peer`'s device that borrows ALL of peer's HIP streams (its own state and buffers otherwise):
 * for callers that keep several models resident and work on them one after the other -- the Kronecker
 * multi-output path keeps its P factorisations this way -- without multiplying the process's hardware queues.
 * Destroy it before `peer`; not for concurrent use with `peer`. */
int gmb_create_sibling(gmb_engine** out, const gmb_engine* peer);
void gmb_destroy(gmb_engine* e);
const char* gmb_last_error(const gmb_engine* e); /* valid until the next call on `e` */
void* gmb_stream(const gmb_engine* e);           /* the hipStream_t launches go to   */

/* -- model definition ------------------------------------------------------------------------
 * gmb_set_data replaces `X, y = self.get_shaped_data("mean")` being captured by the PyMC model
 * (pymc/GP.py:521, 580): X is (N, D) with leading dimension ldx (>= D), y is (N,).  Copies in. */
int gmb_set_data(gmb_engine* e, const double* X, int64_t N, int32_t D, int64_t ldx,
                 const double* y, int32_t memspace);
/* New observations for the SAME inputs (length N): kernel, theta, prepared coordinates and every workspace
 * stay; only the factorisation is invalidated.  No reference counterpart (there the model is rebuilt); used by
 * the Kronecker multi-output path, whose P systems share X and differ in the rotated y (regression/icm.py). */
int gmb_set_y(gmb_engine* e, const double* y, int32_t memspace);

/* Replaces PymcGP._construct_kernels + the noise block of build_model (pymc/GP.py:560-569,
 * 652-729): fixes which columns feed which covariance term. */
int gmb_set_kernel(gmb_engine* e, const gmb_kernel_spec* spec);
int gmb_theta_size(const gmb_kernel_spec* spec);
/* (ABI 12) Periodic continuous kernels (pymc/GP.py:416-447, 676-682).  `periods` holds one period T_d per continuous dimension
 * of the spec (n == n_cont), in the units of X; they are data, not parameters: theta and gmb_theta_size do not change.
 *   mode 0  off (what gmb_set_kernel leaves; `periods` is not read);
 *   mode 1  <kind>+Periodic: the spec's stationary kind applied to the inputs warped by u(x) = (sin(2 pi x / T), cos(2 pi x / T))
 *           per dimension, r^2 = sum_d |u(x_d) - u(x'_d)|^2 / ls_d^2 = sum_d 4 sin^2(pi (x_d - x'_d) / T_d) / ls_d^2
 *           (pm.gp.cov.WarpedInput; the kind keeps its own sqrt(r^2 + 1e-12));
 *   mode 2  pm.gp.cov.Periodic: k = eta^2 exp(-1/2 sum_d sin^2(pi (x_d - x'_d) / T_d) / ls_d^2); the spec's kind must be ExpQuad.
 * Every dimension takes two of the GMB_MAX_DIMS prepared columns, so n_cont <= 8.  GMB_EINVAL for another mode, n != n_cont,
 * n_cont > 8, a period that is not finite and > 0, mode 2 on another kind.  Call it between gmb_set_kernel (which resets the
 * mode to off) and gmb_set_theta: it invalidates theta's prepared coordinates, the resident factor and the inverse factor.
 * Additive models warp every term's own lengthscales with the same periods.  The multi-GPU driver (gmb_dist_*) refuses
 * periodic engines. */
int gmb_set_periodic(gmb_engine* e, int32_t mode, const double* periods, int32_t n);

/* (ABI 16) Change N under the engine; kernel, periods and theta stay, no gmb_set_theta is needed afterwards.
 * gmb_append: K further observations for the SAME kernel and theta: Xnew (K, D) row-major with leading dimension ldx >= D, ynew (K).
 * gmb_truncate: keep the first n_keep observations (1 <= n_keep <= N).
 * Without a valid resident factor they only change the data: the result is what gmb_set_data on the concatenated / cut arrays
 * followed by the stored theta would leave; gmb_factor_valid stays 0.  With a complete, unconsumed single-engine factor they update
 * it: row i of a Cholesky factor depends on rows <= i of Sigma only, so with I0 = floor(min(N_old, N_new) / 128) the block columns
 * [0, I0) are kept and the block rows >= I0 of the bordered matrix are rebuilt, solved against the kept columns, their corner updated
 * (contraction length 128 I0: on the split-k product of gmb_blk_gemm_splitk below when the corner is a handful of tiles or the
 * rule finds slices to cut, on the trailing update's triangular GEMM when an append is so large that the corner has many tiles) and factored; log-det, v and |v|^2 follow.  O(N^2 K) instead of O(N^3).  When
 * the padded row or column count changes, the factor is re-laid to the new leading dimension in a second buffer (the kept triangle
 * copied device to device): a device that cannot hold both returns GMB_ENOMEM with the bytes needed in gmb_last_error before
 * anything is touched.  (Only that buffer is measured up front.  The small allocations behind it -- X, y, v, prepared points: O(N D)
 * -- can still fail after the data has begun to change; the engine then holds no factor and no theta, gmb_num_obs says which N its
 * data has, and gmb_set_data + gmb_set_theta start over.)  Afterwards gmb_factor_valid is 1 and gmb_predict*, gmb_nlml, gmb_copy_* behave as behind gmb_factorize at the
 * new N; everything derived from the old factor (both alphas, U, L^-1, the joint state) is invalid, so the next prediction takes
 * the solve form.  Deterministic call after call; NOT promised to equal a fresh factorisation bit for bit.  GMB_ENOTPD +
 * gmb_notpd_index (a row of the new matrix): the data has the new N, the factor is invalid; gmb_truncate + gmb_factorize recovers.
 * GMB_EINVAL: null pointers, ldx < D, n_keep out of range, no data or theta yet, a consumed factor, distributed or capacity-mode
 * engines, engines whose last factorisation was gmb_dist_*.  K == 0 and n_keep == N are GMB_OK and change nothing. */
int gmb_append(gmb_engine* e, const double* Xnew, int64_t K, int64_t ldx, const double* ynew, int32_t memspace);
int gmb_truncate(gmb_engine* e, int64_t n_keep);
/* N of the data the engine holds now (0 before gmb_set_data), or a negative gmb_status for a null handle: what a binding reads back
 * after gmb_append / gmb_truncate, whatever they returned. */
int64_t gmb_num_obs(const gmb_engine* e);

/* Hyper-parameters on the natural scale -- the role of `point=self.MAP` (pymc/GP.py:846). */
int gmb_set_theta(gmb_engine* e, const double* theta, int32_t n);

/* -- hot path --------------------------------------------------------------------------------
 * gmb_factorize: build Sigma = K(X,X) + noise + jitter*I (lower triangle, HBM-resident), Cholesky
 * factor it in place, forward-solve v = L^-1 y, accumulate sum(log L_ii).  This is what every
 * `pm.find_MAP` objective evaluation (pymc/GP.py:811) and every `Marginal.predict` call
 * (pymc/GP.py:845-847) does first.  Returns GMB_ENOTPD if a pivot is <= 0 or NaN. */
int gmb_factorize(gmb_engine* e);
int64_t gmb_notpd_index(const gmb_engine* e); /* 0-based failing row after GMB_ENOTPD, else -1 */
/* 1 while the engine holds a usable factorisation of the current (data, kernel, theta): after gmb_factorize,
 * and still after gmb_nlml with a gradient (the single-GPU gradient puts the factor's diagonal blocks back);
 * 0 after gmb_set_* or after gmb_dist_nlml with a gradient (which leaves U = L^-T in the factor buffer). */
int gmb_factor_valid(const gmb_engine* e);

/* One objective (+ gradient) evaluation at `theta` in ONE call: gmb_set_theta + gmb_factorize + gmb_nlml, with the gradient's
 * launches enqueued right behind the factorisation's -- no host synchronisation or language round trip in between (at
 * N = 2000 that is 0.1 of 1.5 ms per evaluation of pm.find_MAP's objective, gumbi/regression/pymc/GP.py:811).  Same status
 * codes and side effects as the three calls (GMB_ENOTPD with gmb_notpd_index when the covariance is not positive definite;
 * grad may be NULL), same values bit for bit where the three calls take the same schedules.  One difference: with a gradient,
 * on matrices below 4096 rows and without gmb_set_profiling, no per-phase events are recorded (they cost a tenth of such an
 * evaluation) -- gmb_timings' kbuild_ms / chol_ms / grad_ms then read 0 after this call. */
int gmb_evaluate(gmb_engine* e, const double* theta, int32_t n, double* nlml, double* grad);
/* Negative log marginal likelihood  N/2 log 2pi + sum log L_ii + |v|^2/2  of the last
 * factorisation, and (if grad != NULL, length gmb_theta_size) its gradient w.r.t. natural-scale
 * theta: 1/2 tr((Sigma^-1 - a a^T) dSigma/dtheta).  The factorisation stays valid (gmb_predict may follow
 * without another gmb_factorize).  Priors and Jacobians are added by the Python
 * caller so the MAP formula stays auditable.  Replaces the likelihood part of pm.find_MAP's
 * objective/gradient (pymc/GP.py:580, 811). */
int gmb_nlml(gmb_engine* e, double* nlml, double* grad);

/* Posterior mean and variance at M points -- `Regressor.predict` contract (base.py:477-495),
 * replacing `gp.predict(points_array, point=MAP, diag=True, pred_noise=with_noise)`
 * (pymc/GP.py:845-847).  Xs is (M, D) row-major with leading dimension ldxs; mean/var are
 * caller-allocated length-M arrays in the same memspace as Xs.  Reuses the resident factor. */
int gmb_predict(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise,
                double* mean, double* var, int32_t memspace);

/* (ABI 11) The JOINT posterior at M points (csrc/joint_predict.hpp).  Both calls need the resident factor exactly as gmb_predict
 * does and leave it -- and gmb_nlml, the gradient's leftovers, gmb_factor_valid -- as they found it; V = K(X*, X) L^-T takes the
 * form gmb_predict would take (gmb_set_predict_form) and is held for ALL M points at once (8 * (M padded) * (N padded) bytes, twice
 * in the product form), beside the M x M matrix C.  A request the device cannot hold returns GMB_ENOMEM before anything is
 * launched, with the bytes it needs in gmb_last_error; nothing is written.  Engines with a multi-GPU factorisation (gmb_dist_*,
 * capacity mode) return GMB_EINVAL.  `jitter` (>= 0) is the caller's: PyMC adds its default 1e-6 to a noise-free conditional
 * covariance and nothing when pred_noise=True -- the Python caller passes that convention in, as it does priors and Jacobians.
 *
 * Posterior mean (M) and the full M x M posterior covariance at M points, row-major with leading dimension ldc, both
 * triangles written (exactly symmetric):
 *   C = K(X*,X*) - V V^T  (+ the noise diagonal of the model at X* if with_noise)  + jitter * I
 * pm.gp.Marginal._build_conditional(..., diag=False); diag(C) less noise and jitter is gmb_predict's variance to rounding. */
int gmb_predict_joint(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise, double jitter,
                      double* mean, double* cov, int64_t ldc, int32_t memspace);

/* S joint draws  Y[s, :] = mean + L* Z[s, :],  L* the lower Cholesky factor of the C above (the engine's own factorisation
 * kernels on a second matrix).  Z is S x M standard normals supplied by the caller (row-major, leading dimension ldz), Y is
 * S x M (ldy), mean (M, out) may be NULL.  The draw is a deterministic function of (model, theta, Xs, Z): the same bits call
 * after call.  GMB_ENOTPD + gmb_notpd_index (a row of C) when C is not positive definite; GMB_EHIP when the tile Cholesky
 * abandoned its launch (time-out).  Replaces pm.gp.Marginal.conditional + pm.sample_posterior_predictive at the MAP
 * (gumbi/regression/pymc/GP.py:914-917: draw_point_samples / draw_grid_samples). */
int gmb_draw_joint(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise, double jitter,
                   const double* Z, int64_t S, int64_t ldz, double* Y, int64_t ldy, double* mean, int32_t memspace);

/* (ABI 14) Gradient of the posterior mean with respect to the test point, d mu / d x*, at M points (csrc/predict_grad.hpp) --
 * replaces the autograd pass of the reference's `predict_grad` through its GPyTorch model (gumbi/regression/botorch/GP.py:535-576).
 * In closed form from the prepared coordinates, the factor and alpha = Sigma^-1 y: O(M N d) work in one fused launch per model
 * term, nothing of size M x N is written.  `grad` is M x D row-major with leading dimension ldg >= D, in the memspace of Xs;
 * EVERY column is written: the continuous (and linear) columns of the kernel with the derivative, all others -- categorical
 * columns, the output index -- with 0.  Periodic models differentiate through their warp; additive models sum their terms.
 * Matern-1/2 and Exponential keep PyMC's sqrt(r^2 + 1e-12): their gradient is smooth and 0 at a coincident point.
 * Readiness as gmb_predict (a valid, unconsumed, complete single-engine factor); GMB_EINVAL for bad arguments (ldg < D, ldxs < D),
 * engines with a multi-GPU factorisation (gmb_dist_*) and capacity mode; M == 0 is GMB_OK.  Behind a gradient evaluation
 * (gmb_evaluate / gmb_nlml with grad) it uses that evaluation's alpha; behind a bare gmb_factorize it solves L^T alpha = v once per
 * factorisation by blocked back substitution into a buffer of its own.  The factor, v, alpha (gmb_copy_alpha), the inverse
 * factor, gmb_factor_valid and the joint state are left as found; the same bits call after call.  M is tiled (16384 rows). */
int gmb_predict_grad(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, double* grad, int64_t ldg, int32_t memspace);

/* (ABI 15) Posterior mean and variance at M points WITH their gradients with respect to the test point, d mu / d x* and
 * d sigma^2 / d x* (csrc/predict_grad.hpp): what a gradient-based search of an acquisition function needs per evaluation (the
 * reference's `propose`, gumbi/regression/botorch/GP.py).  mean, var: length M, the values of gmb_predict (solve form); dmean,
 * dvar: M x D row-major with leading dimension ldg >= D, all four in the memspace of Xs.  EVERY column of dmean and dvar is
 * written, categorical columns and the output index with 0, nothing beyond column D.  With W = K(X*, X) Sigma^-1 = V L^-1
 *   d sigma^2 / d x*_d = d k(x*, x*) / d x*_d - 2 sum_n W_mn d k(x*_m, x_n) / d x*_d
 * (the prior term is 2 tau (x*_l - c_l) F_mm for a linear dimension, 0 otherwise); with_noise changes var, not dvar.  Per M-tile:
 * the prediction's cross-covariance and triangular solve, a second blocked triangular pass W = V L^-1 in place, and ONE fused
 * launch per model term for both gradients.  Readiness, refusals and the state contract are gmb_predict_grad's: a complete,
 * unconsumed single-engine factor; GMB_EINVAL for bad arguments, distributed engines and capacity mode; M == 0 is GMB_OK; the
 * factor, v, both alphas, the inverse factor and its flags, the joint state and gmb_factor_valid are left as found; the same bits
 * call after call.  M is tiled as in gmb_predict. */
int gmb_predict_with_grad(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise, double* mean, double* var,
                          double* dmean, double* dvar, int64_t ldg, int32_t memspace);

/* ---- The components of an additive model (csrc/predict_terms.hpp, csrc/term_walk.hpp).  Additive to ABI 16: new functions only.
 * The reference carries `additive_level=` in its signatures and raises NotImplementedError for every level but "total"
 * (gumbi/regression/pymc/GP.py:839-841); these calls go beyond that line.
 *
 * The model's covariance is a sum of T terms, K = sum_t K_t: term 0 the global kernel, term 1 + j the kernel of coregion dimension
 * j of an additive spec (T = 1 otherwise).  Bit t of a `terms` mask selects term t.  Let S be a selection, K_S = sum_{t in S} K_t,
 * and L, v = L^-1 y, alpha = Sigma^-1 y the resident state of the WHOLE model.  Then
 *   mu_S(x*)   = K_S(x*, X) alpha,          V_S = K_S(X*, X) L^-T = sum_{t in S} V_t
 *   cov_S(X*)  = K_S(X*, X*) - V_S V_S^T
 *   cov(f_t, f_u | y)(x*) = -<V_t(x*), V_u(x*)>   for t != u (the priors of different terms are independent).
 * Noise and jitter belong to no term: with_noise adds the model's noise diagonal to a selection's variance, exactly as to the
 * total's (what pm.gp.Marginal.predict(..., given=..., pred_noise=True) would do).
 *
 * terms == 0 or a bit at or beyond T returns GMB_EINVAL and launches nothing.  With all T bits set a *_terms call issues the
 * launches of the call it is named after, in the same order: the same bits.  The selection changes only K(X*, X) and K(X*, X*);
 * behind a gradient evaluation gmb_predict_terms and the joint pair take the product form exactly as their parents do.
 * State contract of all six calls: the factor, v, both alphas, U and the inverse factor with their flags, the joint state and
 * gmb_factor_valid are left as found; the same bits call after call. */

/* T: 1, or 1 + n_coreg for additive specs; a negative status before gmb_set_theta. */
int gmb_num_terms(const gmb_engine* e);

/* gmb_predict for the selection: mean = mu_S, var = diag cov_S (+ noise).  Readiness, tiling and forms as gmb_predict, except that
 * distributed and capacity-mode engines are refused (GMB_EINVAL); M == 0 is GMB_OK.  Beyond pymc/GP.py:839-841. */
int gmb_predict_terms(gmb_engine* e, uint32_t terms, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise,
                      double* mean, double* var, int32_t memspace);

/* gmb_predict_grad for the selection: d mu_S / d x* = sum_{t in S} d K_t(x*, X) / d x* alpha, alpha the whole model's.  Readiness,
 * refusals and layout as gmb_predict_grad.  Beyond pymc/GP.py:839-841. */
int gmb_predict_grad_terms(gmb_engine* e, uint32_t terms, const double* Xs, int64_t M, int64_t ldxs,
                           double* grad, int64_t ldg, int32_t memspace);

/* gmb_predict_joint for the selection: mean = mu_S and C = K_S(X*, X*) - V_S V_S^T (+ the model's noise diagonal if with_noise)
 * + jitter * I.  Arguments, readiness, refusals and memory rule as gmb_predict_joint.  Beyond pymc/GP.py:839-841. */
int gmb_predict_joint_terms(gmb_engine* e, uint32_t terms, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise,
                            double jitter, double* mean, double* cov, int64_t ldc, int32_t memspace);

/* gmb_draw_joint for the selection: Y[s, :] = mu_S + L* Z[s, :] with L* the factor of the C above.  Draws of different selections
 * are draws of their own marginals: they do not add up to one draw of the total.  Beyond pymc/GP.py:839-841. */
int gmb_draw_joint_terms(gmb_engine* e, uint32_t terms, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise, double jitter,
                         const double* Z, int64_t S, int64_t ldz, double* Y, int64_t ldy, double* mean, int32_t memspace);

/* ALL components at M points from one pass: the T blocks V_t are stacked ((T * M padded) x (N padded) doubles, M tiled so that
 * this stays within gmb_predict's 8 GiB rule), solved by ONE triangular solve (always the solve: neither the inverse factor nor U
 * is touched) and reduced without atomics.
 *   means: T rows of M (leading dimension ldm >= M), row t = mu_t = <V_t, v>
 *   cov:   T (T + 1) / 2 rows of M (ldcv >= M), the packed lower triangle of the pointwise T x T posterior covariance of the LATENT
 *          components, row p = t (t + 1) / 2 + u (u <= t):  delta_tu k_t(x*, x*) - <V_t, V_u>  -- no noise, no jitter
 *   noise: M, may be NULL: the model's noise variance at each point (what with_noise adds)
 * The sum of the means is gmb_predict's mean, the sum over the full T x T matrix its noise-free variance, the sum over a
 * selection's rows and columns gmb_predict_terms' -- to rounding.  Nothing beyond column M of a row is written.  Readiness and
 * refusals as gmb_predict_joint (a complete, unconsumed single-engine factor; GMB_EINVAL for distributed and capacity engines);
 * a workspace the device cannot hold returns GMB_ENOMEM before anything is launched; M == 0 is GMB_OK.
 * Beyond pymc/GP.py:839-841. */
int gmb_predict_decompose(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, double* means, int64_t ldm, double* cov,
                          int64_t ldcv, double* noise, int32_t memspace);

/* -- leave-one-out and leave-group-out predictions of the TRAINING rows (added to version 16 without a change of layout) ---------
 * What the model, at the resident theta, predicts for observations it is not shown -- from the resident factorisation alone, no
 * refit (Rasmussen & Williams 5.4.2).  With Sigma = L L^T the factored matrix (noise and jitter on its diagonal) and
 * alpha = Sigma^-1 y:   y_B | y_-B ~ N(y_B - C^-1 alpha_B, C^-1),  C = (Sigma^-1)_BB.  Sigma holds the jitter and gmb_predict's
 * with_noise variance does not, so the jitter is taken off every variance here: with_noise = 1 is gmb_predict(with_noise = 1) on
 * the data without the rows, to rounding.  Beyond the reference, on state only this engine keeps.
 *
 * Readiness and refusals as gmb_predict_joint: a complete, unconsumed single-engine factor; GMB_EINVAL for distributed and
 * capacity-mode engines, a consumed factor, no factorisation yet, null outputs, a range outside [0, N], duplicate or out-of-range
 * idx, m < 1, ldc < m -- nothing launched, nothing written.  A workspace the device cannot hold returns GMB_ENOMEM before anything
 * is launched, the bytes in gmb_last_error.  State contract of the *_terms calls: the factor, v, both alphas, U, L^-1 and their
 * flags, the joint state's meaning and gmb_factor_valid are left as found; the same bits call after call (no atomics). */

/* Leave-one-out predictive mean and variance of the training rows [i0, i0 + n): what the model predicts for observation i from all
 * the others.  mean, var: length n, in `memspace`.  d_i = (Sigma^-1)_ii:
 *   mean_i = y_i - alpha_i / d_i        var_i = 1 / d_i - jitter - (with_noise ? 0 : noise_i)
 * (noise_i: the model's noise variance at row i).  Behind a tile-path gradient evaluation (gmb_evaluate / gmb_nlml with grad:
 * U = L^-T and alpha resident) and unless gmb_set_predict_form(e, 0), d_i = sum_{j >= i} U_ij^2 is ONE pass over the resident
 * triangle (4 N^2 bytes); otherwise selection rows are solved against L in gmb_predict's M-tiles.  n == 0 is GMB_OK. */
int gmb_loo(gmb_engine* e, int64_t i0, int64_t n, int32_t with_noise, double* mean, double* var, int32_t memspace);

/* The JOINT predictive of the m training rows idx[0..m) from all the others.  idx: HOST memory always, distinct, each in [0, N),
 * 1 <= m <= N; outputs in the order of idx.  C = (Sigma^-1)_BB:
 *   mean = y_B - C^-1 alpha_B      cov = C^-1 - jitter I - (with_noise ? 0 : diag noise_B)      var = diag(cov)
 * mean, var: length m; cov: m x m row-major, leading dimension ldc >= m, both triangles, exactly symmetric; cov may be NULL (then
 * nothing of size m x m is formed beyond C's factor), var may be NULL when cov is not.  Always the triangular solve against L; C is
 * factored by the engine's Cholesky on the joint posterior's second matrix: GMB_ENOTPD + gmb_notpd_index (a row of C) when C is
 * not positive definite. */
int gmb_leave_out(gmb_engine* e, const int64_t* idx, int64_t m, int32_t with_noise, double* mean, double* var,
                  double* cov, int64_t ldc, int32_t memspace);

/* -- averages of the posterior over GROUPS of points: marginal effects and contrasts (added to version 16 without a change of
 * layout) -------------------------------------------------------------------------------------------------------------------------
 * fbar_g = sum_{m in g} w_m f(x_m), the weighted mean of the LATENT function over group g of the points (no noise, no jitter), is
 * Gaussian; its variance is w_g^T C w_g with C the joint posterior covariance of the group's points -- not the mean of their
 * variances.  With a_g = sum_{m in g} w_m k(x_m, X) (row g of A, G x N) and Q_gh = sum_{m in g} sum_{m' in h} w_m w_m' k(x_m, x_m'):
 *   V_A = A L^-T        mean = V_A v        cov = Q - V_A V_A^T  (G x G)        var = diag(cov)
 * A and Q are summed by fused kernels that write no covariance row: nothing of size M x M or M x N exists, the device holds
 * O(M D) for the points, 128 x M doubles of one row block of Q's reduction, the task partials, and a prediction's workspace for
 * G (not M) rows.  Beyond the reference.
 *
 * Xs: M x D row-major with leading dimension ldxs >= D, in `memspace`.  offsets: HOST memory always, G + 1 entries,
 * offsets[0] == 0, strictly increasing, offsets[G] == M; group g is rows [offsets[g], offsets[g + 1]) of Xs.  weights: length M,
 * in `memspace`, any sign (a contrast is one group with weights of both signs); NULL = 1 / |g|, a plain mean.  mean, var: length
 * G.  cov: G x G row-major, leading dimension ldc >= G, both triangles, exactly symmetric, its diagonal equal to var; cov may be
 * NULL (then only Q's diagonal is formed: sum |g|^2 pairs instead of M^2), var may be NULL when cov is not.  Variances are NOT
 * clipped.  A group of one point with weight 1 is gmb_predict(with_noise = 0) at that point, to rounding.
 *
 * Readiness and refusals as gmb_predict_joint and the *_terms calls: a complete, unconsumed single-engine factor; GMB_EINVAL for
 * distributed and capacity-mode engines, a consumed factor, no factorisation yet, terms == 0 or a bit at or beyond T, null
 * required pointers, ldxs < D, ldc < G, G < 1, an empty group, offsets that do not start at 0, do not increase strictly or do not
 * end at M, and a weight that is not finite -- the weights are checked on the host for HOST weights only; device-side weights
 * are the caller's to vouch for -- with nothing launched and nothing written.  A request the device cannot hold returns
 * GMB_ENOMEM with the bytes it needs in gmb_last_error before anything is launched or written.  State contract of the *_terms
 * calls: the factor, v, both alphas, U, L^-1 and their flags and gmb_factor_valid are left as found; the joint state's second
 * matrix is used, as gmb_leave_out uses it.  No atomics: the same bits call after call. */
int gmb_predict_groups(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, const int64_t* offsets, int64_t G,
                       const double* weights, double* mean, double* var, double* cov, int64_t ldc, int32_t memspace);
/* ... of the selected terms of an additive model (bit t of `terms` = term t, as the other *_terms calls) */
int gmb_predict_groups_terms(gmb_engine* e, uint32_t terms, const double* Xs, int64_t M, int64_t ldxs, const int64_t* offsets,
                             int64_t G, const double* weights, double* mean, double* var, double* cov, int64_t ldc,
                             int32_t memspace);
/* Host only: the task list the kernels of gmb_predict_groups run over for these offsets -- (group, first point, count) triples,
 * count <= chunk, ascending group, then ascending first point.  Returns the number of tasks and writes at most `cap` triples to
 * `out` (may be NULL); chunk <= 0 = the engine's own (512).  GMB_EINVAL for malformed offsets (as above, with M = offsets[G]). */
int64_t gmb_debug_group_tasks(const int64_t* offsets, int64_t G, int64_t chunk, int64_t* out, int64_t cap);

/* ---- the posterior of the slope d f / d x* : mean, variance and covariance of the partial derivatives (ABI stays 16: new
 * functions only, no change of layout) --------------------------------------------------------------------------------------------
 * The derivative of a GP with a mean-square differentiable kernel is a GP.  Per test point x* (LATENT function: no noise, no
 * jitter) and differentiable model column d, with b_d[n] = d k(x*, x_n) / d x*_d and V_d = b_d L^-T:
 *   dmean_d = V_d v  (= d mu / d x*_d, the quantity gmb_predict_grad returns, by another route)
 *   dcov_de = P_de - V_d V_e,     dvar_d = dcov_dd
 *   P_de    = delta_de sum_t F_t(x*, x*) [ -2 eta_t^2 f'_t(0) J_d^2 + tau_t 1{d linear in t} ]
 * J_d^2 = 1 / ls_d^2 for a stationary kernel (P = eta^2 / ls^2 for ExpQuad, 5 eta^2 / 3 ls^2 for Matern-5/2, 3 eta^2 / ls^2 for
 * Matern-3/2) and w_d^2 (2 pi / T_d)^2 for the periodic forms.  gmb_predict_with_grad's dvar is d sigma^2 / d x*: another quantity.
 *
 * Xs: M x D row-major, leading dimension ldxs >= D, in `memspace`.  dmean, dvar: M x D row-major with leading dimension ldg >= D,
 * every model column; dvar may be NULL.  dcov: NULL, or point m's D x D row-major block at dcov + m * ldc, ldc >= D * D; exactly
 * symmetric, its diagonal equal to dvar.  Rows and columns of model columns that are not differentiable (categories, the output
 * index) are written 0.  Variances are NOT clipped.  What lies between the rows of a strided result is left untouched.
 *
 * A model whose selected terms include a Matern-1/2 or Exponential kernel (<kind>+Periodic with such a kind included) is not
 * mean-square differentiable: GMB_EINVAL, "the process has no derivative", nothing launched.  Readiness and the other refusals
 * are gmb_predict_grad's: a complete, unconsumed single-engine factor; GMB_EINVAL for distributed and capacity-mode engines, no
 * factorisation yet, M < 0, null Xs / dmean, ldxs < D, ldg < D, terms == 0 or a bit at or beyond T (and ldc < D * D).  V is always
 * solved for (as gmb_predict_decompose): the factor, v, both alphas, U, L^-1, their flags and the joint state are left as found,
 * the resident training points hold term 0's preparation on return, and a gmb_predict behind a fit keeps its form and its
 * bits.  No atomics: the same bits call after call. */
int gmb_predict_slope(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, double* dmean, double* dvar, int64_t ldg,
                      double* dcov, int64_t ldc, int32_t memspace);
/* ... of the selected terms of an additive model (bit t of `terms` = term t, as the other *_terms calls) */
int gmb_predict_slope_terms(gmb_engine* e, uint32_t terms, const double* Xs, int64_t M, int64_t ldxs, double* dmean, double* dvar,
                            int64_t ldg, double* dcov, int64_t ldc, int32_t memspace);
/* Host only: test points per M-tile of gmb_predict_slope behind Np (padded) training points with Dc differentiable columns --
 * max(128, mt_max / Dc / 128 * 128), mt_max a prediction's largest M-tile.  GMB_EINVAL for Np < 1 or Dc outside 1 .. 24. */
int64_t gmb_debug_slope_tile_rows(int64_t Np, int32_t Dc);

/* ---- a batch of experiments: greedy integrated variance reduction (ABI stays 16: new functions only, no change of layout) ------
 * Which q of the M candidates Xc, measured next, teach most about the surface over the R reference points Xr?  A GP's posterior
 * covariance does not depend on y: measuring at c lowers the variance at r by cov(c, r)^2 / (var f(c) + noise(c)).  With
 * P = [Xc; Xr] and D = C(Xc, P), the M x (M + R) LATENT posterior covariance, step t = 0 .. q - 1 is
 *   s_a    = D[a, a] + noise_a                       (noise_a: what gmb_predict(with_noise = 1) adds at candidate a; 0 without)
 *   gain_a = sum_r w_r D[a, M + r]^2 / s_a           (candidates with s_a <= 0 or not finite, or masked: excluded)
 *   picks[t] = argmax gain_a (ties: lowest index), gains[t] = its gain
 *   D[a, p] -= (D[c, a] * D[c, p]) * (1 / s_c)       for all a, p, c = picks[t]
 * allow_repeats = 0 masks a picked candidate; with allow_repeats = 1 and noise it may be picked again (a replicate).  When no
 * candidate has a positive finite gain the loop stops: the remaining picks are -1, their gains 0.
 *
 * Xc: M x D and Xr: R x D row-major with leading dimensions ldc, ldr >= D; w: R weights >= 0, NULL = 1 / R each; picks, gains: q
 * values; score0 (M values, may be NULL): the step-0 gain of every candidate (0 for an excluded one) -- q = 0 computes only
 * these; ivar0 (may be NULL): sum_r w_r var f(r) before any pick, by the prediction's own variance reduction.  All in `memspace`.
 *
 * Readiness is gmb_predict_joint's: a complete, unconsumed single-engine factor.  GMB_EINVAL with a text for M < 1, R < 1, q < 0,
 * null Xc / Xr (picks / gains with q > 0), ldc < D, ldr < D, a negative or non-finite weight and a NaN coordinate (device-side
 * arguments are copied to the host for these checks).  The candidates must fit one M-tile of a prediction (V within 8 GiB, at
 * most 32768 rows); that, and a request the device cannot hold, return GMB_ENOMEM with the bytes in gmb_last_error before
 * anything is launched or written.  The factor, v, both alphas, U, L^-1, their flags and the joint state are left as found.  No
 * atomics, fixed-order sums: the same bits call after call. */
int gmb_design_batch(gmb_engine* e, const double* Xc, int64_t M, int64_t ldc, const double* Xr, int64_t R, int64_t ldr,
                     const double* w, int32_t q, int32_t with_noise, int32_t allow_repeats, int64_t* picks, double* gains,
                     double* score0, double* ivar0, int32_t memspace);
/* Host only: the plan of gmb_design_batch behind Np (padded) training points.  Writes at most `cap` values to `out` (may be
 * NULL) and returns how many there are: Mc (padded candidates), ld (doubles per row of D), mt_max, mt (rows of the prediction
 * workspace), ntile, nchunk, the step kernel's chunk (columns) and rows per workgroup, the bytes of the call's own buffers for
 * D = 1, q = 0; then per point tile (first stacked index, count, padded count, first column of D); then per column chunk
 * (first column, end).  A refusal returns -(code): 1 M < 1, 2 R < 1, 3 Np no positive multiple of 128, 4 the candidates exceed
 * one M-tile, 5 R > 2^30. */
int64_t gmb_debug_design_plan(int64_t Np, int64_t M, int64_t R, int64_t* out, int64_t cap);

/* ---- joint posteriors of many small batches, with derivatives (ABI stays 16: new functions only, no change of layout) ----------------
 * What a reparameterised Monte-Carlo batch acquisition (q-EI; the reference's `propose(q=..)`, gumbi/regression/botorch/GP.py:652)
 * needs for R restarts at once (csrc/predict_batches.hpp).  Xs: (B q) x D row-major, leading dimension ldxs >= D, in `memspace`;
 * batch b is rows [b q, (b + 1) q), 1 <= q <= 16.  Everything is the LATENT posterior (no noise) against the resident factor:
 *   mean   B q values
 *   cov    B x q x q contiguous: C_b = K(P_b, P_b) - V_b V_b^T + jitter I, both triangles written, exactly symmetric
 *   dmean  (B q) x D with leading dimension ldg >= D: gmb_predict_grad's quantity
 *   dcov   B x q x q x D contiguous: dcov[b, j, l, :] = d C_b[j, l] / d x_j; for l = j the FULL derivative of C_b[j, j], which is
 *          gmb_predict_with_grad's dvar at that point.  With w_l = Sigma^-1 k(X, x_l), per term and summed over the terms,
 *            d C[j, l] / d x_j = d_1 k(x_j, x_l) - sum_n W_ln d k(x_j, x_n) / d x_j                 (l != j)
 *            d C[j, j] / d x_j = d k(x_j, x_j) / d x_j - 2 sum_n W_jn d k(x_j, x_n) / d x_j
 *          (the same f' and sqrt(r^2 + 1e-12) as gmb_predict_grad: two coincident points of a batch give a Matern-1/2 derivative 0)
 * Categorical and output columns of dmean and dcov are 0.  dmean and dcov may BOTH be NULL: only the values are computed, and
 * W = V L^-1 is not formed (the same mean and cov bits).  Per M-tile the flow is gmb_predict_with_grad's; tiles are cut at whole
 * batches.  The contractions over the training points run on v_mfma_f64_16x16x4_f64, one wave per (batch, chunk of N), partials
 * summed in chunk order: no atomics, the same bits call after call.  Readiness, refusals and the state contract are
 * gmb_predict_with_grad's; GMB_EINVAL also for q outside 1 .. 16, B < 0, a NULL mean or cov, dmean without dcov or the reverse;
 * B == 0 is GMB_OK; a request the device cannot hold returns GMB_ENOMEM.  A refusal launches nothing and writes nothing. */
int gmb_predict_batches(gmb_engine* e, const double* Xs, int64_t B, int32_t q, int64_t ldxs, double jitter, double* mean, double* cov,
                        double* dmean, int64_t ldg, double* dcov, int32_t memspace);
/* Host only: the plan of gmb_predict_batches behind N training points padded to Np.  Writes at most `cap` values to `out` (may be
 * NULL) and returns how many there are: bt (batches of a full M-tile), ntile, mt (rows of the prediction workspace), slots
 * ((chunk, batch) pairs the partials are sized for), the unit of a chunk's length; then per tile (first batch, batches, points,
 * padded points, chunk length, chunks).  A refusal returns -(code): 1 q outside 1 .. 16, 2 B < 1, 3 N < 1 or Np no multiple of
 * 128 that holds N, 4 B q > 2^40. */
int64_t gmb_debug_batch_plan(int64_t N, int64_t Np, int64_t B, int32_t q, int64_t* out, int64_t cap);

/* ---- pathwise posterior draws: function samples by Matheron's rule (ABI stays 16: new functions only, no change of layout) ------------
 * csrc/pathwise.hpp, csrc/paths_plan.hpp.  For draw s, with a prior draw from F random Fourier features in the prepared coordinates
 * u = x / ls,
 *   f_s(x) = phi(x)^T w_s + k(x, X) a_s,   a_s = Sigma^-1 (y - Phi(X) w_s - d o eps_s),   phi_f(x) = eta sqrt(2 / F) cos(omega_f^T u + b_f),
 * d^2 = sigma^2 + jitter, exactly the diagonal the covariance build adds to K.  The draws are of the LATENT function.
 * gmb_paths_prepare: omega F x Dc row-major (Dc continuous dimensions, in the order of the kernel's idx_cont), phase F, w S x F and
 * eps S x N standard normals, all HOST arrays.  Forms A = Sigma^-1 R for all S draws with a prediction's two triangular passes
 * against the resident factor and keeps it on the device, tied to the factorisation: any later call that changes data, theta or
 * the factor makes the paths stale (GMB_EINVAL from the evaluations).  1 <= S <= 512, 1 <= F <= 16384.  Readiness is
 * gmb_predict_batches's (a current single-engine factor); GMB_EINVAL -- nothing launched, nothing written -- also for models with
 * linear dimensions, coregion tables (categorical dimensions, an output column), additive or periodic models.  The factor, both
 * alphas, U, the inverse factor and the joint state are left as found.
 * gmb_paths_eval: all S draws at the M rows of Xs (leading dimension ldxs >= D, in `memspace`): Y is S x M row-major with leading
 * dimension ldy >= M.  No triangular pass, nothing of size M x N: M is walked in tiles of 65536 points.
 * gmb_paths_eval_own: point m on draw draw[m] (int32, in `memspace`, in [0, S): anything else is GMB_EINVAL before any launch) only:
 * val M values and, unless grad is NULL, grad M x D with leading dimension ldg >= D (columns that are no continuous dimension: 0).
 * Fixed-order sums, no atomics: the same bits call after call.  M == 0 is GMB_OK; a request the device cannot hold returns
 * GMB_ENOMEM before any launch.  gmb_paths_clear drops the state and frees its buffers. */
int gmb_paths_prepare(gmb_engine* e, int32_t S, int32_t F, const double* omega, const double* phase, const double* w, const double* eps);
int gmb_paths_eval(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, double* Y, int64_t ldy, int32_t memspace);
int gmb_paths_eval_own(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, const int32_t* draw, double* val, double* grad, int64_t ldg,
                       int32_t memspace);
int gmb_paths_clear(gmb_engine* e);
/* S of the prepared draws (the rows gmb_paths_eval writes), 0 when none are prepared; a stale set still counts until it is replaced
 * or cleared. */
int32_t gmb_paths_count(gmb_engine* e);
/* Host only: the plan of the pathwise calls for S draws of F features at M points behind N training points.  Writes at most `cap`
 * values to `out` (may be NULL) and returns how many there are: Sp (S padded to 16), draw blocks of 64, N and F padded to 4, rows
 * of the largest M-tile, M-tiles, doubles of the all-draws partials, doubles of the own-draw partials for `nacc` accumulators;
 * then per tile (first point, points, padded points, point tiles of 16, chunk length and chunks of the all-draws kernel, chunk
 * length and chunks of the own-draw kernel).  A refusal returns -(code): 1 S outside 1 .. 512, 2 F outside 1 .. 16384, 3 M < 1 or
 * beyond 2^40, 4 N < 1 or beyond 2^40. */
int64_t gmb_debug_paths_plan(int64_t N, int64_t F, int64_t M, int64_t S, int32_t nacc, int64_t* out, int64_t cap);

/* ---- sparse GPs: the FITC approximation on m inducing points (ABI stays 16: new functions only, no change of layout) -----------------
 * PyMC's MarginalSparse(approx="FITC") (gumbi/regression/pymc/GP.py:571-591, fit(sparse=True, n_u=...)), csrc/fitc.hpp.  With Z the
 * m inducing points and k the model's covariance without noise:
 *   Kuu = k(Z, Z) + jitter I = Lu Lu^T      A = Lu^-1 k(Z, X)      lambda_i = max(k(x_i, x_i) - sum_k A_ki^2, 0) + sigma^2
 *   B = I + A Lambda^-1 A^T = L_B L_B^T     c = L_B^-1 A Lambda^-1 y
 *   NLML = 1/2 sum log lambda_i + sum log diag(L_B) + 1/2 (y^T Lambda^-1 y - c^T c) + N/2 log 2 pi
 *   predict: As = Lu^-1 k(Z, X*), C* = L_B^-1 As:  mean = As^T L_B^-T c,  var = k** - colsum(As^2) + colsum(C*^2) (+ sigma^2)
 * An evaluation costs O(N m^2) and holds O(m^2 + m * tile + N) on the device: X is walked in column tiles (gmb_debug_fitc_plan),
 * nothing of N x N elements exists and none of the exact path's buffers is allocated or touched.  Fixed-order sums, no atomics: the
 * same bits call after call.
 *
 * Models: one output, no categorical dimensions (n_coreg == 0, out_col == -1), not additive, no linear dimensions, not periodic;
 * every stationary kind, ARD or a shared lengthscale, scalar noise.  Everything else, and distributed or capacity-mode engines:
 * GMB_EINVAL with a text that names the limit. */

/* The inducing points: Z is m x D row-major (D of gmb_set_data) with leading dimension ldz >= D, in `memspace`; copied in and prepared
 * by the path of the data and the test points.  1 <= m <= 16384.  Needs gmb_set_data and gmb_set_kernel; a later gmb_set_data,
 * gmb_set_kernel or gmb_set_periodic drops the points.  Allocates the O(m^2) state (GMB_ENOMEM with the bytes when the device cannot
 * hold it). */
int gmb_fitc_set_inducing(gmb_engine* e, const double* Z, int64_t m, int64_t ldz, int32_t memspace);

/* One objective (+ gradient) evaluation of the FITC marginal likelihood at `theta` (length gmb_theta_size: [ls | eta | sigma]); grad
 * may be NULL.  Sets theta exactly as gmb_set_theta does: an exact factor resident on the same engine is stale afterwards
 * (gmb_factor_valid == 0) and is neither used nor overwritten.  GMB_ENOTPD with gmb_notpd_index (a row of the m x m matrix) when
 * Kuu or B is not positive definite.  Leaves Lu, L_B, c and L_B^-T c resident for gmb_fitc_predict.  The gradient is hand-written
 * reverse mode over the same tiles; each tile's block A is formed again in that pass instead of being kept (O(m * tile) memory). */
int gmb_fitc_evaluate(gmb_engine* e, const double* theta, int32_t n, double* nlml, double* grad);

/* Mean and variance of the FITC posterior at M points against the state the last gmb_fitc_evaluate left resident; arguments as
 * gmb_predict.  GMB_EINVAL when there is none: before any evaluation, or when theta (gmb_set_theta, gmb_evaluate), the data
 * (gmb_set_data, gmb_set_y, gmb_append, gmb_truncate) or the inducing points changed since.  M is tiled as the columns of X are; a
 * point's result does not depend on where in the call it stands.  M == 0 is GMB_OK. */
int gmb_fitc_predict(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise, double* mean, double* var,
                     int32_t memspace);

/* Host only: the plan of gmb_fitc_evaluate for N observations and m inducing points.  Writes at most `cap` values to `out` (may be
 * NULL) and returns how many there are: Np, mp, mr (N, m, m + 1 padded to 128), columns of X per tile, columns of the widest tile,
 * tiles, partial-sum blocks of the column kernels; the bytes of the buffer list for D = 1 in three parts -- what depends on m alone,
 * the m x tile blocks, the per-column vectors; then per tile (first column, count, padded count).  A refusal returns -(code):
 * 1 N < 1, 2 m < 1, 3 m > 16384, 4 N > 2^40. */
int64_t gmb_debug_fitc_plan(int64_t N, int64_t m, int64_t* out, int64_t cap);

/* ---- GP classification: a latent GP with a logit link and a Bernoulli likelihood by the Laplace approximation (ABI stays 16: new
 * functions, one new status and one new struct, no change of layout) ---
 * The reference's GPC (gumbi/regression/pymc/GP.py:759-797, pymc/extras.py:8-66) without sampling: Rasmussen & Williams, Algorithms
 * 3.1, 3.2 and 5.1, csrc/laplace.hpp.  Labels y in {0, 1} (what gmb_set_data / gmb_set_y hold), Sigma exactly the matrix gmb_factorize
 * builds (K + the noise entries of theta + jitter I; a classifier passes sigma = 0), zero mean:
 *   pi = 1 / (1 + e^-f)   log p(y | f) = sum y f - log(1 + e^f)   g = y - pi   W = pi (1 - pi)   s = sqrt(W)
 *   mode: from a = f = 0 in EVERY call (no warm start), b = W f + g, B = I + (s s^T) o Sigma = L L^T,
 *         a^ = b - s o B^-1 (s o (Sigma b)), a <- a + t (a^ - a), f = Sigma a, t = 1 halved while Psi(a, f) = -1/2 a^T f + log p(y | f)
 *         falls below the previous Psi (slack 1e-14 |Psi|); stop at max |f_new - f| <= tol max(1, max |f_new|)
 *   -log q(y | theta) = -Psi(a^, f^) + sum log L_ii with B at the mode
 *   gradient: 1/2 tr((Z' - a' a'^T) dSigma/dtheta) by the trace pass of gmb_evaluate, Z' = R + u u^T, a' = a^ + u,
 *         R = (s s^T) o B^-1, s2 = -1/2 (1 - diag B^-1)(1 - 2 pi), u = s2 - R (Sigma s2)   (no division: valid where W is 0)
 * Caps: 40 Newton iterations, 20 halvings per iteration; hitting one is GMB_ENOCONV, never a silent result.  Resident N x N matrices:
 * Sigma, the factor buffer (B, then its factor) and, with the gradient, the inverse's -- the exact path's two plus one.  Fixed-order
 * sums, no floating-point atomics: the same bits call after call.
 *
 * Models: whatever a non-additive, single-output gmb_evaluate accepts.  Additive specs, an output column (n_out > 1, heteroskedastic
 * noise), periodic mode, distributed and capacity-mode engines: GMB_EINVAL.
 *
 * State: a Laplace call leaves B's factor in the factor buffer, so the exact path is "not factored" behind it (gmb_factor_valid == 0:
 * gmb_predict and its relatives refuse until gmb_factorize / gmb_evaluate), and every exact factorisation drops the Laplace state. */

typedef struct gmb_laplace_stats {
  int32_t iterations; /* accepted Newton steps of the last gmb_laplace_evaluate */
  int32_t halvings;   /* halvings of t over all of them */
  double psi;         /* Psi at the last accepted iterate */
  double step;        /* max |f_new - f| of the last accepted step */
} gmb_laplace_stats;

/* -log q(y | theta) and, unless grad is NULL, its gradient; theta and the gradient are laid out as gmb_evaluate's.  Sets theta as
 * gmb_set_theta does.  GMB_EINVAL: labels that are not exactly 0 or 1 (checked on the device), a model outside the scope above;
 * GMB_ENOTPD + gmb_notpd_index: B not positive definite, or non-finite values; GMB_ENOCONV: a cap was hit; GMB_ENOMEM with the bytes
 * before anything is computed.  After an error no Laplace state is resident and the engine is usable. */
int gmb_laplace_evaluate(gmb_engine* e, const double* theta, int32_t n, double* nlq, double* grad);

/* Latent mean k*^T (y - pi^) and variance k** - |L^-1 (s o k*)|^2 at M points (k** without noise and jitter, as
 * gmb_predict(with_noise = 0)); arguments as gmb_predict.  Valid only behind a successful gmb_laplace_evaluate with nothing in between
 * that changes the data, the labels, the kernel or theta (gmb_set_*, gmb_append, gmb_truncate, gmb_factorize, gmb_evaluate,
 * gmb_fitc_evaluate): otherwise GMB_EINVAL with a text that names the cause.  M == 0 is GMB_OK. */
int gmb_laplace_predict(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, double* mean, double* var, int32_t memspace);

/* The Newton iteration of the last gmb_laplace_evaluate (also one that ended in GMB_ENOCONV). */
int gmb_laplace_info(const gmb_engine* e, gmb_laplace_stats* out);

/* The resident mode: f^ and a^ (f^ = Sigma a^), each Np = N rounded up to 128 doubles on the host, 0 beyond N; either may be NULL.
 * Readiness as gmb_laplace_predict. */
int gmb_laplace_copy_mode(const gmb_engine* e, double* f, double* a);

/* tol > 0 (default 1e-9) and 1 <= max_iter <= 40 (default 40) of the Newton iteration. */
int gmb_laplace_set_options(gmb_engine* e, double tol, int32_t max_iter);

/* Host only: the plan of gmb_laplace_evaluate for N observations (csrc/laplace_plan.hpp).  Writes at most `cap` values to `out` (may be
 * NULL) and returns how many there are: Np, Nr, block rows nt, workspace slots of the symmetric product (tiles of the lower triangle),
 * partial sets of the likelihood pass, doubles per slot, sums per set, bytes of the state's own buffers; then per block row the nt + 1
 * offsets (in doubles) of the parts its sum adds, in order.  A refusal returns -(code): 1 N < 1, 2 N > 2^22. */
int64_t gmb_debug_laplace_plan(int64_t N, int64_t* out, int64_t cap);

/* Test door: out = Sigma v by the symmetric product against the resident Sigma of the last gmb_laplace_evaluate; v and out are Np
 * doubles on the host (entries of v beyond N are not read as data: they count as 0).  Readiness as gmb_laplace_predict. */
int gmb_debug_laplace_symv(gmb_engine* e, const double* v, double* out);

/* Pairwise-distance extrema used for the lengthscale prior (gumbi/utils/gp_utils.py:15-48):
 * for each group (one per column if ard, else all n_cols jointly) the minimum NON-ZERO and the
 * maximum Euclidean distance over all N(N-1)/2 pairs; lower[g] = -1 if every pair coincides.
 * X is (N, n_cols) row-major, host memory.  Runs on `device`. */
int gmb_ls_limits(int32_t device, const double* X, int64_t N, int32_t n_cols, int64_t ldx,
                  int32_t ard, double* lower, double* upper);

/* -- introspection --------------------------------------------------------------------------- */
int gmb_set_profiling(gmb_engine* e, int32_t on); /* per-launch hipEvent timing of GEMMs */
int gmb_timings_get(const gmb_engine* e, gmb_timings* out);

/* Microbenchmark: sustained v_mfma_f64_16x16x4_f64 rate of `device` in TFLOP/s (register-only
 * kernel, no memory traffic) -- the measured denominator for the MFMA roofline -- and the shader
 * cycles one wave spends per MFMA (64 = the datasheet issue rate; wall rate / this = clock). */
int gmb_mfma_f64_peak(int32_t device, double* tflops, double* cycles_per_mfma);
/* The same register-only loop launched back to back for `seconds` (<= 60; 37 ms per launch): mean and worst
 * per-launch rate and the shader clock in MHz the loop ran at (2 x s_memtime span / launch duration: the counter
 * ticks every second shader cycle on gfx950) -- the sustained
 * ceiling under the box's power management, to be sampled before AND after a timed region. */
int gmb_mfma_f64_sustained(int32_t device, double seconds, double* mean_tflops, double* min_tflops,
                           double* shader_mhz, int64_t* launches);

/* Copy out pieces of the resident state (tests / multi-GPU driver):
 *   rows [r0, r0+nr) x cols [c0, c0+nc) of the factor buffer (lower triangle meaningful),
 *   written row-major into `out` (nr*nc doubles, host). */
int gmb_copy_factor(const gmb_engine* e, int64_t r0, int64_t nr, int64_t c0, int64_t nc,
                    double* out);
int gmb_copy_v(const gmb_engine* e, double* out); /* v = L^-1 y, length N, host */
/* alpha = Sigma^-1 y (length N, host); exists after gmb_nlml with a gradient.  Used by the
 * Kronecker (ICM) multi-output path, whose outer chain rule needs it (gumbi_amd/regression/icm.py). */
int gmb_copy_alpha(const gmb_engine* e, double* out);

/* -- kernel-level doors (tests, tuning tools; device pointers, column-major) -------------------
 * The leaf, strip-solve and MFMA GEMM kernels of the factorisation on caller-provided blocks, so
 * that each can be checked against LAPACK on its own.  All matrices are column-major float64 in
 * device memory with the given leading dimensions; sizes must be multiples of 128. */
/* Host-only: the tile list of one MFMA GEMM launch exactly as the kernel enumerates it (XCD-balanced runs,
 * triangular skipping, strided rows, longest-first and L2-aware strip orders); out = (block, tm, tn) triples,
 * *grid = the launch's grid size; returns the number of triples. */
int64_t gmb_debug_tile_list(int32_t mt, int32_t nt, int32_t bm, int32_t bn, int32_t k, int32_t tri,
                            int32_t tri_off, int32_t nblk_stride, int32_t klo_n, int32_t khi_n, int32_t order,
                            int32_t strip, int32_t* out, int64_t cap, int32_t* grid);
/* Host-only: the tiles of one covariance-build launch exactly as cov_tile_kernel enumerates them (strips of `strip`
 * tiles of a tile row per workgroup; tri_grid: lower triangle of a ti x tj tile grid; row_stride > 0: one rank's
 * block rows row_first, row_first + row_stride, ...; otherwise the ti x tj rectangle, XCD-remapped unless
 * keep_order); out = (block, tile row, tile column) triples, *grid = the launch's grid size; returns the count. */
int64_t gmb_debug_cov_grid(int32_t ti, int32_t tj, int32_t strip, int32_t tri_grid, int32_t row_first,
                           int32_t row_stride, int32_t keep_order, int32_t* out, int64_t cap, int64_t* grid);
/* Host-only: ticket t of the persistent tile Cholesky (csrc/chol_tiles.hpp; column-major over the lower block triangle of
 * an nrt x nct block grid) -> its tile (*I, *J); returns the number of tasks of that grid (t out of range: I = J = -1). */
int64_t gmb_debug_chol_task(int32_t t, int32_t nct, int32_t nrt, int32_t* I, int32_t* J);
/* Persistent tile Cholesky: switch the per-task wall-clock stamps of the FOLLOWING factorisations on (1) / off (0) / leave
 * them (-1) and, when `out` is not NULL, copy the stamps of the last one: 4 uint64 per task -- ticks of the 100 MHz wall
 * clock at: ticket taken / contraction done / solve input ready / tile published -- tasks in ticket order, at most
 * cap_tasks of them.  Returns the number of tasks of the last tile factorisation (0: the last factorisation used another
 * schedule or recorded nothing), or a negative gmb_status. */
int64_t gmb_chol_task_trace(gmb_engine* e, int32_t enable, uint64_t* out, int64_t cap_tasks);
/* Fault injection for the tests: the NEXT persistent tile factorisation starts its ticket counter at `n`, i.e. the tiles of
 * tickets 0 .. n-1 are never computed and every other task ends up waiting for one of them.  The launch must notice (bounded
 * waits: a few seconds), drain, and gmb_factorize must return GMB_EHIP -- never hang the GPU.  One shot. */
int gmb_debug_chol_lose_tickets(gmb_engine* e, int32_t n);
/* Timing tools only (tools/gpu_dist_emulate.py): declare the last factorisation -- single-engine, replicated or capacity --
 * valid whatever it produced, so that the gradient / prediction passes can be TIMED behind a factorisation that ran on a fake
 * transport (garbage numbers, the real launch and collective pattern) and ended with GMB_ENOTPD.  Their results are garbage
 * too.  GMB_EINVAL when no factorisation was attempted since the last gmb_set_theta. */
int gmb_debug_assume_factored(gmb_engine* e);
/* Schedule of the Cholesky for the following factorisations: -1 = by size (default), 0 = plain recursion, launches only,
 * 2 = masked look-ahead, 3 = persistent tile kernel, 4 = plain recursion whose bottom panels (<= 16 block columns with every
 * row below them) are single launches of the tile kernel -- what matrices beyond the tile kernel's range (224 block columns)
 * take by size since ABI 10.  Returns the previous setting PLUS ONE (0 = by size, 1 = recursion, 3, 4, 5), so that no valid
 * answer collides with a negative gmb_status.
 * (gmb_debug_assume_factored, ABI 10: GMB_EINVAL unless GUMBI_HIP_DEBUG_DOORS=1 is set in the environment.) */
int gmb_set_chol_scheme(gmb_engine* e, int32_t scheme);
/* Schedule of the gradient's inverse and Sigma^-1 for the following evaluations: -1 = by size (default: tile tasks for the
 * matrices the tile Cholesky factors, fused into the factorisation's launch by gmb_evaluate), 0 = the launch tree (recursive
 * block inversion, GEMM launches), 1 = tile tasks in a launch of their own behind the factorisation, 2 = fused whenever the
 * tile Cholesky runs.  `lag` >= 0: in the fused launch the inverse's tasks of block column c - lag follow the factorisation's
 * tasks of column c in the ticket order (negative: keep the current value).  Returns the previous scheme plus one, or a
 * negative gmb_status. */
int gmb_set_grad_scheme(gmb_engine* e, int32_t scheme, int32_t lag);
/* Host-only: the task list of the persistent evaluation launch for an nrt x nct block grid (csrc/eval_tiles.hpp):
 * word = kind << 30 | I << 15 | J, kind 0 = Cholesky tile (I, J), 1 = tile (I, J) of U = L^-T, 2 = tile (I, J) of
 * Sigma^-1; `with_chol` = the factorisation's tasks are part of the launch, `lag` = how many block columns the inverse
 * follows the factorisation by.  Writes at most `cap` words, returns the number of tasks. */
int64_t gmb_debug_eval_tasks(int32_t nct, int32_t nrt, int32_t with_chol, int32_t lag, uint32_t* out, int64_t cap);
/* (ABI 9) `with_chol` bit 1 of gmb_debug_eval_tasks: the Sigma^-1 tasks in PAIRS -- a task word whose J field carries 0x4000 stands
 * for the two tiles (I, J) and (I, J + 1), J + 1 <= I, computed in one pass over block row I of U (128 x 256: the task's own
 * operand row is streamed once for two tiles).  gmb_set_eval_pairs: -1 = by size (default: matrices of at least 72 block
 * columns), 0 = never, 1 = always; same results to the bit either way; returns the previous mode plus one, or a negative
 * gmb_status. */
int gmb_set_eval_pairs(gmb_engine* e, int32_t mode);
/* How gmb_predict forms A^T = K(X*, X) L^-T (pm.gp.Marginal.predict's `solve_lower`, pymc/GP.py:845-847).  Behind a gradient
 * evaluation on the tile path (N <= ~28k: gmb_evaluate, or gmb_nlml with a gradient) the engine still holds U = L^-T of the
 * resident factor; the prediction is then ONE product with a triangular operand (the GEMM that runs at 0.93 of the f64 matrix
 * peak) instead of a triangular solve (0.73 at N = 10k).  -1 = that whenever U is there (default), 0 = always solve, 1 = as -1.
 * Only the variance uses the inverse factor; the mean is K(X*, X) alpha with the gradient's alpha (refined against L to the
 * accuracy of a triangular solve).  Tested against an extended-precision reference up to cond(Sigma) ~ 3e9
 * (tests/test_gpu_conditioning.py): the mean's error within 1.25 x that of the solve form on the same factor, the variance within
 * the solve form's bar; and <= 1e-10 relative to the solve form on the golden cases.  Returns the previous mode + 1. */
int gmb_set_predict_form(gmb_engine* e, int32_t form);
/* (ABI 10) Allocate now what the following calls would allocate on first use: the factor buffer (8 Nr Np bytes: 80 GB at
 * N = 100k), with `gradient` != 0 the Sigma^-1 buffer of gmb_nlml / gmb_evaluate (8 Np^2 bytes), with M > 0 the workspaces of
 * gmb_predict for M points.  Needs gmb_set_data + gmb_set_kernel + gmb_set_theta.  No reference counterpart: a caller that times a
 * first call (bench.py's one-step side figures) takes the tens of gigabytes of hipMalloc out of it. */
int gmb_reserve(gmb_engine* e, int32_t gradient, int64_t M);
/* The covariance build alone: what gmb_factorize factors -- the lower-triangle 128 x 128 tiles of
 * Sigma = K + noise + jitter (pymc/GP.py:580), row N = y, identity padding -- written column-major into `out`
 * (device memory; ceil((N+1)/128)*128 rows x ceil(N/128)*128 columns, leading dimension ldo >= the row count).
 * Needs data, kernel and theta; the resident factor is left alone.  Entries above the tile diagonal are not written. */
int gmb_blk_covariance(gmb_engine* e, double* out, int64_t ldo);
/* Factor one 128 x 128 diagonal block in place (lower triangle; columns >= nvalid are identity
 * padding and are left alone).  dinv16 (optional, 8 x 256 doubles) receives the column-major
 * inverses of the eight 16 x 16 diagonal sub-blocks of the identity-padded factor: the operands
 * gmb_blk_trsm and gmb_blk_invert need.  *logdet_accum += sum log L_cc; *info = first bad pivot. */
int gmb_blk_potrf(gmb_engine* e, double* Akk, int64_t lda, int32_t nvalid, double* dinv16,
                  double* logdet_accum, int32_t* info);
/* invLkk (128 x 128 column-major, identity-padded) = inverse of a block factored by gmb_blk_potrf. */
int gmb_blk_invert(gmb_engine* e, const double* Lkk, int64_t lda, int32_t nvalid,
                   const double* dinv16, double* invLkk);
/* B <- B inv(Lkk)^T in place: B is nrows x 128 (nrows a multiple of 16, leading dimension ldb);
 * rows / columns >= nvalid of the block act as identity whatever the buffer holds there. */
int gmb_blk_trsm(gmb_engine* e, double* B, int64_t ldb, int64_t nrows, const double* Lkk,
                 int64_t ldl, const double* dinv16, int32_t nvalid);
/* C[n + m*ldc] = beta*C + alpha * sum_k A[m + k*lda] * B[n + k*ldb];  tri != 0 skips tiles that
 * lie strictly above the diagonal of the (n, m) index space shifted by tri_shift tiles. */
int gmb_blk_gemm_nt(gmb_engine* e, double* C, int64_t ldc, const double* A, int64_t lda,
                    const double* B, int64_t ldb, int64_t m, int64_t n, int64_t k, double alpha,
                    double beta, int32_t tri, int64_t tri_shift);
/* (ABI 13) The same product with every field of the launch's descriptor and every choice the launcher makes in the caller's
 * hands, so that a test can run each kernel form on its own (tests/test_gpu_gemm.py).  Column-major, device pointers:
 *   C[nc(i) + j*ldc] = beta * C[..] + alpha * sum_{k in [k_lo, k_hi)} A[j + k*lda] * B[nb(i) + k*ldb],   i < n, j < m
 * nb(i) / nc(i) = (i / 128) * stride * 128 + i % 128 with stride = nblk_stride (B; 0 = 1) and cblk_stride (C; 0 = as B).
 * Per TILE (tm, tn) of the block tile BM x BN the launch runs:  R = (row of the tile's first n index with stride krow_stride, 0 =
 * as B) + krow_off;  k_hi = khi_n ? min(k, R + BN) : k;  k_lo = klo_m*tm*BM + klo_n*R clamped to [0, k_hi];  with tri the tile
 * is skipped (C untouched) when nb(first i) + BN - 1 + tri_off < tm*BM.  C == B selects the in-place form (m == 128, ldc == ldb).
 * Pins: -1 leaves the choice to the launcher; a pinned combination the launcher could not produce itself (C prefetch with
 * beta == 0, in place or on the 128 x 128 tile; LDS-DMA staging on another tile or in place; order 1 / 2 where the launcher's
 * rule excludes them; a strip on a launch the rule gives none; the in-place form on the 64 x 64 tile or with m != 128) returns
 * GMB_EINVAL and launches nothing.  *launched (may be NULL) = what ran:  bits 0-1 variant | bit 2 LDS-DMA | bit 3 C prefetch |
 * bit 4 in place | bits 5-6 order | bits 8-15 strip | bits 16-30 grid size (saturating at 0x7fff); 0 when nothing was launched. */
typedef struct gmb_gemm_desc {
  int64_t ldc, lda, ldb, m, n, k;   /* m, n multiples of 128, k of 16 */
  double alpha, beta;
  int32_t tri, tri_off;             /* tri_off in elements (a multiple of 32) */
  int32_t nblk_stride, cblk_stride;
  int32_t klo_m, klo_n, khi_n, krow_off, krow_stride;
  int32_t variant;                  /* -1 = the launch model's choice; 0 = 128 x 128, 1 = 64 x 64, 2 = 128 x 64, 3 = 128 x 32 */
  int32_t staging;                  /* -1 = engine default; 0 = register-staged; 1 = LDS-DMA (variant 0 only) */
  int32_t pfc;                      /* -1 = by the launcher's rule (beta != 0, k <= 1024, out of place); 0 / 1 = pin */
  int32_t order;                    /* -1 = by the rule; 0 / 1 / 2 = pin */
  int32_t strip;                    /* -1 = by the rule; >= 0 = pin (m-tiles per strip, <= 255) */
} gmb_gemm_desc;
int gmb_blk_gemm_ex(gmb_engine* e, double* C, const double* A, const double* B, const gmb_gemm_desc* d,
                    int32_t* launched);
/* (ABI 16) The same product for FEW output tiles and a LONG contraction, split along k (csrc/gemm_splitk.hpp): m, n multiples of 128,
 * k of 16, tri != 0 skips the tiles strictly above the diagonal.  Two launches in stream order: the grid (slices x computed tiles)
 * writes each slice's 128 x 128 partial to an engine workspace laid out [tile][slice][128 * 128]; the second adds a tile's partials in
 * ascending slice order and applies alpha and beta.  No atomics, nothing waits: the same bits call after call.  `slices` = -1: by the
 * rule -- a function of (tile count, k) alone: min(256 / tiles, k / 256), at least 1, slices equal multiples of 16 with a shorter last
 * one; >= 1 pins the number.  *slices_used (may be NULL) = what ran, 0 when nothing was launched.  GMB_EINVAL, nothing launched: bad
 * sizes, more than 65535 computed tiles (it is the kernel for FEW tiles), or a pinned `slices` that leaves a slice empty or not a
 * multiple of 16. */
int gmb_blk_gemm_splitk(gmb_engine* e, double* C, int64_t ldc, const double* A, int64_t lda, const double* B, int64_t ldb,
                        int64_t m, int64_t n, int64_t k, double alpha, double beta, int32_t tri,
                        int32_t slices /* -1 = by the rule, >= 1 = pin */, int32_t* slices_used);
/* -- ONE GP over the GPUs of a node (no reference counterpart -- the reference is
 * single-process; the work replaced is what pm.find_MAP / Marginal.predict do per evaluation,
 * pymc/GP.py:811, 845-847) -------------------------------------------------------------------------------
 * One process per GPU, every process holds an engine with the SAME data / kernel / theta.  128-row blocks
 * of the covariance matrix are dealt round-robin over the ranks (1-D block-cyclic rows); the native driver
 * (gumbi_amd/csrc/dist_driver.hpp) runs the panel loop with look-ahead on this rank's HIP streams and
 * exchanges data through ONE collective, an all-gather of float64 buffers in device memory:
 *   all_gather(ctx, send, recv, count, stream): every rank contributes `count` doubles at `send`; `recv`
 *   receives world * count doubles in rank order; the operation is ordered on the hipStream_t `stream`
 *   (enqueue it there, or synchronise the stream, move the data and return).  0 = success.
 * gmb_rccl_comm_create gives the production transport (RCCL over xGMI: ncclAllGather on a communicator of
 * its own; librccl is resolved with dlopen -- pass the path of the copy the process already uses, or NULL
 * for the loader's); callers may supply any other transport with the same contract (the tests use gloo). */
typedef struct gmb_comm {
  int32_t rank, world;
  void* ctx;
  int32_t (*all_gather)(void* ctx, const void* send, void* recv, int64_t count, void* stream);
} gmb_comm;

int gmb_rccl_unique_id(const char* librccl_path, void* id128);  /* rank 0: 128 bytes to hand to every rank */
int gmb_rccl_comm_create(gmb_comm** out, const char* librccl_path, const void* id128, int32_t rank,
                         int32_t world, int32_t device);         /* collective: ncclCommInitRank          */
void gmb_rccl_comm_destroy(gmb_comm* c);
int gmb_rccl_comm_ranks(const gmb_comm* c); /* ncclCommCount of the communicator (what RCCL itself reports) */
/* (ABI 10) 1 when the transport holds TWO communicators over the same ranks (the second split off the first with ncclCommSplit):
 * RCCL executes the collectives of one communicator in issue order whatever their streams, so the driver's collectives on the
 * communication stream (a panel column's TAIL, the gradient's chunks) would hold up the main stream's; with two, the engine's main
 * stream (declared by every gmb_dist_* call) and every other stream have their own.  0: one communicator (ncclCommSplit missing or failed, or GUMBI_RCCL_ONE_COMM set): correct, serialised. */
int gmb_rccl_comm_split(const gmb_comm* c);
const char* gmb_rccl_last_error(void);

/* The schedule one rank executes, as data (host-only, no device needed): step kinds
 *   0 KBUILD  covariance tiles of the rank's block rows
 *   1 SQUARE  all-gather the block rows [lo, hi) = [c0, c1) of the panel's diagonal square (`elems` doubles
 *             per rank: maxcount * 128 rows x (c1 - c0) * 128 columns), then factor it locally
 *   6 SOLVE   solve the rank's block rows in [lo, hi) = [c1, nrt) of the panel against the square (no communication)
 *   2 PANEL   all-gather the HEAD of the solved panel column: block rows [lo, hi) = [c1, min(c1 + w, nrt)) -- the rows of the next
 *             panel's square, all the chain needs from the other ranks -- on the main stream (`elems` as for SQUARE)
 *   7 TAIL    all-gather the rest of the panel column, block rows [lo, hi) = [c1 + w, nrt), on the communication stream
 *             (`stream` = 2) beside the next panel's chain; only the bulk update reads it          (6, 7: since ABI 10)
 *   3 UPDATE  A[rows, lo:hi] -= L[rows, c0:c1] L[lo:hi, c0:c1]^T on the rank's block rows >= lo, on stream
 *             `stream` (0 main, 1 bulk)
 *   4 FORK    the bulk stream waits for everything issued on the main stream so far (and for the TAIL issued since the last
 *             FORK);  5 JOIN  the main stream waits for the bulk stream
 * (first, count): the rank's block rows first, first + world, ... of the step's row range. */
typedef struct gmb_dist_step {
  int32_t op, c0, c1, lo, hi, first, count, maxcount, stream;
  int64_t elems;
} gmb_dist_step;
/* number of steps (the first min(cap, n) are written to out; out may be NULL) or a negative gmb_status;
 * panel_blocks <= 0 selects the default panel width */
int64_t gmb_dist_plan(int64_t N, int32_t rank, int32_t world, int32_t panel_blocks, gmb_dist_step* out,
                      int64_t cap);

/* How the ranks of gmb_dist_* hold the factor.  0 (default) = REPLICATED: compute is partitioned by block rows, every rank
 * ends with the complete factor in a full-size buffer (N = 100k: 80 GB per rank whatever the number of GPUs).  1 = CAPACITY
 * (csrc/dist_capacity.hpp): a rank keeps only its own block rows + two column-panel buffers; the gradient and the prediction
 * stream L through again, panel by panel from its owners -- "N beyond one GPU" (N = 200k over 8 GPUs: ~160 GB per rank).
 * Same results (other grouping of some sums).  Takes effect with the next gmb_dist_factorize; returns the previous mode or a
 * negative gmb_status.  gmb_copy_factor is not available on a capacity-mode engine (no rank holds the factor). */
int gmb_dist_set_mode(gmb_engine* e, int32_t mode);
/* Device bytes the engine holds through its own allocations right now (peak != 0: the largest value so far). */
int64_t gmb_resident_bytes(const gmb_engine* e, int32_t peak);

/* gmb_factorize over comm->world ranks (collective: every rank calls it with the same state).  Every rank
 * ends with the complete factor (replicated mode; its own block rows in capacity mode), v, log-det and -- on failure -- the
 * same GMB_ENOTPD / gmb_notpd_index. */
int gmb_dist_factorize(gmb_engine* e, const gmb_comm* comm, int32_t panel_blocks);
/* gmb_nlml over the ranks; with grad != NULL the inverse, Sigma^-1 and the trace reductions are
 * partitioned by block rows and every rank receives bit-identical (nlml, grad). */
int gmb_dist_nlml(gmb_engine* e, const gmb_comm* comm, double* nlml, double* grad);
/* gmb_predict with the M points sharded over the ranks; every rank passes the same Xs and receives the
 * complete mean / var. */
int gmb_dist_predict(gmb_engine* e, const gmb_comm* comm, const double* Xs, int64_t M, int64_t ldxs,
                     int32_t with_noise, double* mean, double* var, int32_t memspace);

#ifdef __cplusplus
}
#endif
#endif /* GUMBI_HIP_H */
