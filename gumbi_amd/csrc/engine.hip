// engine.hip -- host side of libgumbi_hip.so: the C ABI of include/gumbi_hip.h.
//
// One engine = one HIP device + one stream + the resident state of one GP:
//   raw inputs X (N x D), y; prepared coordinates (scaled / shifted / categorical, SoA);
//   the covariance / factor buffer A (column-major, (N+1 rounded up to 128) rows x (N rounded up
//   to 128) columns) whose row N carries y and, after factorisation, v = L^-1 y;
//   inv(L_kk) for every 128 x 128 diagonal block; predict workspaces.
//
// Cholesky: recursive over block columns -- chol(c0,c1) = chol(c0,mid); trailing update
// A[mid:END, mid:c1] -= L[mid:END, c0:mid] L[mid:c1, c0:mid]^T on f64 MFMA; chol(mid,c1).
// Most flops land in GEMMs with k >= N/4, so the update is MFMA- rather than HBM-bound.
// Leaves: potrf_leaf (factor + invert a diagonal block) then the panel solve as a GEMM with
// inv(L_kk).  Predict: V = K(X*,X) L^-T by the same recursion on V's columns.
//
// There is no CPU fallback anywhere in this file: without a HIP device every entry point
// returns GMB_ENODEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <functional>
#include <unordered_map>
#include <mutex>
#include <memory>
#include <vector>

#include "../../include/gumbi_hip.h"
#include "device_buffers.hpp"
#include "workspaces.hpp"
#include "term_walk.hpp"
#include "factor_state.hpp"
#include "eval_plan.hpp"
#include "kernel_dispatch.hpp"
#include "covariance.hpp"
#include "gemm_f64.hpp"
#include "gemm_splitk.hpp"
#include "gradient.hpp"
#include "potrf_leaf.hpp"
#include "trsm_strip.hpp"
#include "chol_tiles.hpp"
#include "eval_tiles.hpp"
#include "predict_form.hpp"
#include "joint_predict.hpp"
#include "predict_grad.hpp"
#include "predict_terms.hpp"
#include "leave_out.hpp"
#include "group_average.hpp"
#include "predict_slope.hpp"
#include "design_batch.hpp"
#include "pathwise.hpp"
#include "predict_batches.hpp"
#include "fitc.hpp"
#include "laplace.hpp"

using namespace gmb;

namespace {

constexpr int DIST_MAX_WORLD = 64;   // ranks one GP can be spread over (status words of gmb_dist_*)
constexpr int DIST_MAX_PAYLOAD = 7;  // scalars that travel with a status word (dist_agree)
constexpr int DIST_HEADER = 3;       // words in front of them: status | collectives issued so far | hash of their sequence

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// what a timed launch is, for ev_collect's sums; the values are written into GMB_TRACE_FILE lines and never change
enum EvKind : int {
  EV_CHOL_PANEL_GEMM = 0,   // Cholesky: in-panel product of the latency-bound chain
  EV_LEAF = 1,              // potrf leaf
  EV_CHOL_SOLVE_GEMM = 2,   // Cholesky: product of a panel's triangular solve (multi-GPU drivers)
  EV_PREDICT_GEMM = 3,      // prediction (the tile triangular solve included)
  EV_GRAD_GEMM = 4,         // gradient
  EV_CHOL_STRIP = 5,        // Cholesky: strip solve below a leaf
  EV_SOLVE_STRIP = 6,       // strip solve of the prediction's / the gradient's triangular solve
  EV_CHOL_UPDATE = 7,       // Cholesky: bulk trailing update
  EV_CHOL_TILES = 8,        // the persistent tile Cholesky, whole matrix
  EV_EVAL_TILES = 9,        // the persistent evaluation launch
  EV_CHOL_TILES_PANEL = 10, // the tile kernel on a panel at the recursion's bottom
  // (ABI 14) launches that are no products: logged to GMB_TRACE_FILE while profiling, counted in no field of gmb_timings
  EV_PREDICT_COV = 11,        // a prediction's cross-covariance launch K(X*, X) (first term)
  EV_PREDICT_GRAD = 12,       // gmb_predict_grad: the partial + finishing launches of one term
  EV_PREDICT_GRAD_ALPHA = 13, // gmb_predict_grad: the back substitution for alpha
  // (ABI 15)
  EV_PREDICT_VGRAD = 14,      // gmb_predict_with_grad: the fused partial + finishing launches of one term
  EV_PREDICT_VGRAD_SOLVE = 15, // gmb_predict_with_grad: the second triangular pass W = V L^-1 of one M-tile
  // (ABI 16)
  EV_SPLITK = 16,             // the split-k product's launch pair (gemm_splitk.hpp): flags = slices
  EV_TERM_GRAM = 17,          // gmb_predict_decompose: the reduction's partial + final launches of one M-tile (k = terms)
  EV_GROUP_COV = 18,          // gmb_predict_groups: the partial launches of one reduction of one term (mt = column blocks, nt = tasks,
                              // flags = 0 the cross part A, 1 the prior part Q, 2 its diagonal only)
  EV_SLOPE_COV = 19,          // gmb_predict_slope: the derivative cross-covariance launch of the first selected term (mt x nt tiles
                              // of 128 x 128 pairs, k = differentiable columns written per pair)
  EV_DESIGN = 20,             // gmb_design_batch: a PHASE, around the launches listed above (flags = 0 the solved rows V of one point
                              // tile, 1 its prior + rank-N update, 2 the greedy loop: mt = candidates, nt = doubles per row of D, k = picks)
  EV_FITC = 21,               // the sparse path's own launches (mt x nt tiles of the block): flags = 0 a cross-covariance against Z, 1 a
                              // pass V L^-1, 2 a column / row / adjoint / transpose pass over a block, 3 a derivative reduction or the
                              // prediction's reduction
  EV_BATCH = 23,              // gmb_predict_batches: the contraction launches of one M-tile (mt = batches, nt = chunks, k = q; flags = 0
                              // the partial + finishing launches of Q = V V^T, 1 those of one term's derivative sums)
  EV_PATHS = 24,              // the pathwise draws' own launches (mt = point tiles or point blocks, nt = chunks, k = draws; flags = 0 the
                              // all-draws kernel + its finish over the features at the training points (prepare), 1 the all-draws
                              // kernel + its finish of one M-tile (eval), 2 the own-draw kernel + its finish; the residual and A's
                              // transposed store of a preparation are in no event)
  EV_LAPLACE = 22             // gmb_laplace_evaluate: a PHASE, around the launches listed above (mt = block rows, k = Newton iteration;
                              // flags = 0 the build of Sigma, 1 a build of B or Z', 2 a Cholesky with its two vector solves, 3 a symmetric
                              // matrix-vector product, 4 elementwise and likelihood work, 5 the inverse, 6 the trace pass)
};
inline bool ev_trace_only(EvKind k) { return k == EV_PREDICT_COV || (k >= EV_PREDICT_GRAD && k <= EV_PATHS); }

struct EventPair {
  hipEvent_t a, b;
  hipStream_t s;  // the stream the pair was opened on: ev_end closes it there
  EvKind kind;
  double flops;
  int mt, nt, k, flags;
  bool masked = false;  // launched on the CU-masked bulk stream
};

}  // namespace

constexpr int GACC_REGION = 64 + MAX_TABS * GMB_MAX_LEVELS * GMB_MAX_LEVELS + 64;  // gradient accumulators of one covariance term
constexpr int GACC_DOUBLES = (1 + GMB_MAX_COREG) * GACC_REGION;  // additive models: one region per term
// the engine's scalar block, ONE allocation (one memset per evaluation): [0, 64) scalars ([0] log-det, [1] |v|^2, [2 ..] the partials
// and arrival counter of the |v|^2 sum) | [64, 72) the failure index (int32) | [72, ...) the gradient accumulators + 64 of scratch
constexpr int SCAL_INFO_AT = 64, SCAL_GACC_AT = 72, SCAL_DOUBLES = SCAL_GACC_AT + GACC_DOUBLES + 64;

// The matrix a Cholesky / triangular-solve host routine works on, said by its caller: the training factor (train_factor), the
// joint posterior's C (joint_factor_ref), a panel window of the capacity driver (cap_window).  A VIEW: the buffers and their
// capacities stay with their owner; only the tile kernel's control block is reached as its owner's buffer, because the
// launches grow it (reserve).
struct FactorRef {
  double* A;          // column-major, leading dimension ld: Sigma's lower triangle in, L out
  int64_t ld;
  int64_t N, Np, Nr;  // order; padded to 128; rows of the bordered layout ((N + 1) up)
  double* dinv16;     // 8 x (16 x 16) sub-block inverses per diagonal block
  double* scal;       // head of a scalar block: [0] log-det, the info word (int32) at SCAL_INFO_AT
  DevBuf<uint32_t>* ct;  // control block of the persistent tile kernel
  int32_t* info() const { return reinterpret_cast<int32_t*>(scal + SCAL_INFO_AT); }
};

// what the tile kernel did in a factorisation, for the caller that has to look at it afterwards
struct CholResult {
  bool tiles = false;     // it ran (whole matrix, panels, or the fused evaluation launch): the abort word has to be read back
  bool traced = false;    // ... and left task stamps in dct_trace
  bool injected = false;  // ... with injected faults (its failure is reported, not retried)
  int ntasks = 0;         // tasks of the whole-matrix launch
};

struct gmb_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;

  // data
  int64_t N = 0, Np = 0, Nr = 0, ld = 0;
  int32_t D = 0;
  DevPool pool;  // every device block of this engine (device_buffers.hpp); gmb_destroy frees them through it
  DevBuf<double> dX, dy, dA;
  DevBuf<double> dDinv16;  // 8 x (16 x 16) sub-block inverses per diagonal block (triangular solves)

  // kernel + parameters
  gmb_kernel_spec spec{};
  bool have_spec = false, have_theta = false;
  std::vector<double> theta;
  int nc_pad = 1;
  int periodic = 0;        // gmb_set_periodic: 0 off, 1 <kind>+Periodic, 2 pm.gp.cov.Periodic; the prepared columns are then 2 n_cont
  double periods[8] = {};  // T_d per continuous dimension (standardized units)
  PreparedPoints pts;  // the training points as the covariance kernels read them (SoA, stride = rows)
  DevBuf<double> dtabs, dnoise;
  // The model's covariance terms (apply_theta; empty until gmb_set_theta): terms[0] is the global kernel -- the ONLY copy of its
  // parameters, and the preparation the resident points hold between calls -- and an additive model adds term 1 + j, the kernel
  // of coregion dim j.  Covariances are built and differentiated term by term (accumulating passes: walk_terms).
  struct Term {
    PrepArgs pa;
    CovParams cp;
    double eta;
    int n_tab_acc;  // tables whose partials this term's gradient pass produces
  };
  std::vector<Term> terms;
  std::vector<double> htabs;  // host copies (gradient chain rule)
  std::vector<double> hnoise;

  // factorisation results
  DevBuf<double> dscal;     // the scalar block (SCAL_DOUBLES, uncounted): [0] logdet, [1] |v|^2, [2..] partials of that sum
  int32_t* dinfo = nullptr; // = dscal + SCAL_INFO_AT (and dgpart = dscal + SCAL_GACC_AT)
  DevBuf<double> dv;
  FactorState fs;                // what of the last factorisation is resident and valid (factor_state.hpp)
  DevBuf<double> dDiagSave;      // the factor's diagonal blocks while the gradient keeps U in their place
  DevBuf<double> dsk;            // partials of the split-k product (gemm_splitk.hpp): [tile][slice][128 * 128]
  int64_t notpd = -1;
  double logdet = 0.0, vnorm2 = 0.0;

  // the workspaces (workspaces.hpp: each writes its members once, for the allocation and for the guards' measurement alike)
  PredictWorkspace pw;     // what an M-tile of Mt rows needs (predict_workspace)
  // GEMM-form prediction (predict_form.hpp): U = L^-T behind a tile-path gradient sits in the factor buffer's upper triangle +
  // dUdiag; the first prediction transposes it into dW's lower triangle, every one until the next factorisation is one GEMM into dV2
  int predict_form = -1;   // -1 = GEMM form whenever U is there; 0 = always the triangular solve; 1 = as -1 (explicit)
  GemmFormWorkspace pw2;   // its second V
  JointState jt;           // the second matrix of gmb_predict_joint / gmb_draw_joint (joint_predict.hpp)
  DevBuf<double> dpart;    // the prediction's chunked partial sums (2 x chunks x the rows asked for: predict_buffers)
  // gmb_predict_grad (predict_grad.hpp): workspaces of its own -- a prediction's (Mt x Np and friends) stay as they are --
  // and alpha by back substitution for the states in which no gradient evaluation left one
  PredictGradWorkspace pg;
  DevBuf<double> pg_part;
  DevBuf<double> dalpha_bs;  // Np: alpha, then Np: the running right-hand side
  // gmb_predict_with_grad: the variance gradient of an M-tile (its partials are a second set in pg_part)
  DevBuf<double> vg_grad;
  TermsWorkspace tg;        // gmb_predict_decompose (predict_terms.hpp), beside a prediction's workspace of T stacked blocks
  GroupWorkspace ga;        // gmb_predict_groups (group_average.hpp); beside it the task partials and the call's index arrays
  DevBuf<double> ga_part;   // [task][column] of one reduction
  SlopeWorkspace slope;     // gmb_predict_slope (predict_slope.hpp), beside a prediction's workspace of Dc stacked blocks
  DevBuf<int64_t> ga_idx;   // the task triples, then first_task (G + 1), then offsets (G + 1)
  BatchWorkspace bw;        // gmb_predict_batches (predict_batches.hpp), beside a prediction's and gmb_predict_grad's workspaces
  PathState paths;          // gmb_paths_* (pathwise.hpp): A = Sigma^-1 R of the prepared draws, tied to the factor's epoch
  DesignWorkspace dz;       // gmb_design_batch (design_batch.hpp), beside a prediction's workspace of one point tile
  FitcState fitc;           // the sparse (FITC) path: everything it keeps (workspaces.hpp), nothing of it shared with the exact path
  LaplaceState lap;         // GP classification (laplace.hpp): Sigma and the vectors; B's factor sits in the factor buffer, FactorState "not factored"

  // gradient workspace
  DevBuf<double> dW;     // Np x Np column-major: L^-1 then Sigma^-1
  DevBuf<double> dalpha;
  double* dgpart = nullptr;   // = dscal + SCAL_GACC_AT: accumulators of the trace reductions (GACC_DOUBLES) + 64 doubles of scratch
  DevBuf<double> dgred;       // per-workgroup partial vectors of grad_tile_kernel (two-stage, fixed-order sums)
  DevBuf<double> dgbig;       // per-wave copies of coregion tables with more than 8 levels

  // cached launch plan of the batched levels of the triangular inverse (static per data set)
  struct InvLevelPlan {
    int variant[2] = {0, 0};     // tile shape of the T^T and W21 batches
    int grid_x[2] = {0, 0};
    int count = 0;               // nodes on this level
    int64_t off[2] = {0, 0};     // first descriptor of each batch in dplan_gemm
    int64_t toff = 0;            // first transpose job in dplan_tr
    int tr_rows = 0, tr_cols = 0;  // largest transpose
    double flops[2] = {0.0, 0.0};
  };
  std::vector<InvLevelPlan> inv_plan;  // indexed by depth; count == 0 -> level not batched
  DevBuf<GemmArgs> dplan_gemm;  // (uncounted, as dplan_tr)
  DevBuf<TransposeJob> dplan_tr;
  int64_t plan_N = -1, plan_ld = -1, plan_Np = -1;
  const double* plan_W = nullptr;
  const double* plan_A = nullptr;
  bool batch_inverse = true;
  bool lpt_order = true;
  long long lpt_max_tiles = 16384;  // launches with more 128 x 128 tiles than this keep the L2-aware strip order (GMB_LPT_MAX_TILES)
  int cov_strip = 0;   // GMB_COV_STRIP: tiles per workgroup of the covariance build (0 = by size)
  int tile_strip = 8;  // GMB_TILE_STRIP: m-tiles per strip of the L2-aware tile order (0 = row-major runs)

  // timing
  bool profiling = false;
  gmb_timings tm{};
  std::vector<EventPair> evs;
  bool naive_leaf = false;
  bool gemm_dma = true;   // the 128 x 128 launches stage their operands by LDS-DMA (gemm_f64_dma_kernel); GMB_GEMM_DMA=0: the
                          // register-staged double buffer (tools/gpu_ab_gemm_dma.py)
  bool small_tiles = true;
  int gemm_variant = 0;
  long long wg_slots = 512;  // resident GEMM workgroups: two per compute unit
  bool force_variant = false;  // tuning: GMB_GEMM_VARIANT pins the tile shape of every out-of-place GEMM

  // concurrency inside one factorisation / gradient: the launch helpers take their stream as an argument; the orchestrators
  // pass `stream`, except the look-ahead Cholesky (bulk updates on aux[2]) and the level-parallel triangular inverse
  // (independent merges dealt over stream + aux[0..2])
  hipStream_t aux[3] = {nullptr, nullptr, nullptr};
  // -1 = by size; 0 = plain recursion; 2 = masked look-ahead; 3 = persistent tile kernel (chol_tiles.hpp)
  int chol_scheme = -1;
  // persistent tile Cholesky: control words + per-tile flags (zeroed before every launch), optional task trace
  DevBuf<uint32_t> dct;
  DevBuf<unsigned long long> dct_trace;
  bool ct_trace = false;
  CholResult chol;           // what the tile kernel did in the last TRAINING factorisation
  int ct_lose = 0;           // fault injection (gmb_debug_chol_lose_tickets): one shot
  // a factorisation that has been enqueued but not checked yet (factorize_enqueue / factorize_finish): where its scalars
  // land on the host, and the events around its two phases
  // (PINNED host memory: an asynchronous copy into pageable memory makes the host wait for the stream, and the gradient of
  // gmb_evaluate would be enqueued only after the factorisation has finished -- 80 us of idle GPU per evaluation at N = 2000)
  struct HostLanding {
    double scal[2];
    int32_t info;
    uint32_t abort;
    double gacc[GACC_DOUBLES];  // gmb_evaluate's light path: the gradient accumulators land here too (eval_land_kernel)
  };
  HostLanding* hl = nullptr;
  HostLanding* hl_dev = nullptr;  // the same memory as the device addresses it
  hipEvent_t fe[4] = {nullptr, nullptr, nullptr, nullptr};  // K-build begin / end, Cholesky begin / end
  // (how one evaluation uses them -- the fused `light` path, the launch that clears instead of a memset, whether the events are
  // recorded -- is an EvalPlan, made by gmb_evaluate and passed down in a FactorJob: eval_plan.hpp)
  int inline_prep_max_rows = 4096;  // small evaluations: the covariance build prepares the points itself (CovTileArgs::inline_prep)
  // persistent evaluation launch (eval_tiles.hpp): L^-T by rows and Sigma^-1 as tile tasks, fused with the tile Cholesky
  // when the caller asks for the gradient together with the factorisation (gmb_evaluate)
  int grad_scheme = -1;        // -1 = by size; 0 = launch tree (winv_levels); 1 = tile tasks behind the factorisation; 2 = fused
  int et_lag = -1;             // the INV tasks of column c - lag follow the CHOL tasks of column c in the task list (-1: by size)
  DevBuf<uint32_t> det_tasks;  // task list on the device, and what it was built for
  int et_key[5] = {-1, -1, -1, -1, -1};
  int et_pairs = -1;           // Sigma^-1 tasks of two tiles (128 x 256; eval_tiles.hpp: et_zz2_task): -1 = by size, 0 = off, 1 = on
  int et_pairs_min_blocks = 72;  // (measured, profiles/r05_eval_pairs_ab.txt: +19 % at 24 block columns, +8 % at 41, 0 at 50 - 64,
                                 //  -0.7 % at 79, -1.0 ... -1.2 % at 128 - 157: a pair halves the number of tasks the tail is balanced with)
  int et_ntasks = 0;
  DevBuf<double> dUdiag;       // diagonal tiles of U = L^-T
  DevBuf<double> dApart;       // partial products U(r,c) v_c
  int et_min_blocks = 1;       // smallest matrix (in 128-blocks) whose MAP evaluation runs as the fused launch by default
  // the bottom of the plain recursion (matrices beyond tiles_max_blocks): panels of <= panel_tiles_w block columns, with every
  // row below them, are factored by ONE launch of the tile kernel instead of leaf / strip / small-product launches
  // (chol_tiles_panel).  chol_factor asks chol_cols for them, i.e. the single-engine recursion
  // only: the multi-GPU driver's chains run beside a bulk stream whose workgroups a persistent launch would not fit beside.
  // Width by A/B on one box at N = 50k (profiles/r06_panel_tiles_ab.txt): launches only 598 ms; 4: 600, 8: 594.5, 16: 591, 32: 594 --
  // the panel launch does the in-panel work at the bulk updates' rate (73 TF/s-equivalent, chain included); what it takes away
  // is the ~500 launch boundaries of the leaves, strips and small products.
  int panel_tiles_w = 16;
  bool panel_tiles_veto = false;
  int tiles_min_blocks = 6, tiles_max_blocks = 224;  // matrices (in 128-blocks) the tile kernel factors by default (measured faster from N = 768 on)
  int tiles_trsm_min_blocks = 16;                    // ... and the tile triangular solve of the predict path (measured from N = 2560 on)
  int masked_max_blocks = 128;  // GMB_MASKED_MAX_BLOCKS: largest matrix (in 128-blocks) factored with the masked bulk stream
  std::vector<hipEvent_t> sync_pool;
  size_t sync_next = 0;
  bool lookahead = true;
  bool par_inverse = true;
  bool aux_shared = false;  // aux[2] is the process-wide masked stream (not ours to destroy)
  bool aux_borrowed = false;  // aux[0..2] belong to the engine this one was created beside (gmb_create_sibling)
  int part_cus = 0;         // compute units the masked stream leaves free
  // multi-GPU driver (dist_driver.hpp): packed send / receive staging of the all-gathers
  DevBuf<double> dsend, drecv;
  DevBuf<double> dsend2, drecv2;  // ... and of the panel columns' TAILs, which travel on the communication stream beside the next chain
  int panel_blocks = 8;
  bool panel_auto = true;  // panel width grows with the matrix (GMB_PANEL_BLOCKS pins it)
  // Multi-GPU driver, CAPACITY mode (gmb_dist_set_mode(e, 1); dist_capacity.hpp): no rank holds the whole factor.  dAown =
  // this rank's block rows, packed ((owned blocks * 128) rows x Np columns); dPanel = one column panel of L with ALL its rows
  // (what a panel all-gather delivers), addressed through a virtual full-buffer base so that every kernel written for the
  // replicated layout works on it unchanged -- two of them (the factorisation's look-ahead; the gradient: one panel of L and
  // one column chunk of U = L^-T with all its rows).
  int dist_mode = 0;
  DevBuf<double> dAown;
  int64_t ld_own = 0;
  int own_world = -1, own_rank = -1;  // what dAown holds the rows of
  DevBuf<double> dPanel;
  // gmb_predict's triangular solve V <- V L^-T, when somebody else has to do it (the capacity driver streams L through)
  std::function<int(double*, int64_t, int)> solve_hook;
  DevBuf<double> dstat;     // (uncounted) status words (+ payload) the ranks exchange: this rank's, then everybody's (dist_agree)
  // Every collective this engine has issued on a transport, in host issue order: count and a running hash of (element count,
  // stream).  RCCL matches the collectives of a communicator by ISSUE ORDER on every rank -- and gmb_dist_nlml issues them on
  // two streams -- so the ranks compare these two words whenever they agree on a status: a rank that issued a different
  // sequence is reported instead of silently pairing the wrong buffers.
  uint64_t coll_count = 0, coll_hash = 0;
  std::vector<hipEvent_t> time_pool;  // timing events of the multi-GPU driver's communication probes
  size_t time_next = 0;
};

namespace {

int fail(gmb_engine* e, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (e) e->err = buf;
  return code;
}

#define HIP_TRY(e, call)                                                              \
  do {                                                                                \
    hipError_t _s = (call);                                                           \
    if (_s != hipSuccess)                                                             \
      return fail(e, GMB_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_s), \
                  __FILE__, __LINE__);                                                \
  } while (0)

// Device memory of an engine: every block belongs to the engine's DevPool (device_buffers.hpp) and is held by a DevBuf field of
// gmb_engine / JointState, by a row group of such fields, or by a ScopedBuf on the stack.  A buffer is declared once and sized
// where it is used, with reserve (keep what is large enough), renew (always a fresh block) or a group's reserve(rows); nothing
// else has to know about it: the pool keeps the byte count (gmb_resident_bytes: what the multi-GPU driver's capacity mode is
// judged by) and gmb_destroy frees whatever is live.  What the pool could not get is reported here.
int alloc_refused(void* owner, size_t bytes, const char* why) {
  return fail(static_cast<gmb_engine*>(owner), GMB_ENOMEM, "hipMalloc of %lld bytes failed: %s", (long long)bytes, why);
}

// ---- timing helpers -----------------------------------------------------------------------
struct PhaseTimer {
  gmb_engine* e;
  hipEvent_t a = nullptr, b = nullptr;
  explicit PhaseTimer(gmb_engine* e_) : e(e_) {
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    (void)hipEventRecord(a, e->stream);
  }
  void stop() { (void)hipEventRecord(b, e->stream); }
  double ms() {  // caller has synchronised the stream
    float t = 0.f;
    (void)hipEventElapsedTime(&t, a, b);
    return (double)t;
  }
  ~PhaseTimer() {
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
  }
};

void ev_begin(gmb_engine* e, hipStream_t s, EvKind kind, double flops, int mt = 0, int nt = 0, int k = 0, int flags = 0) {
  if (!e->profiling) return;
  EventPair p;
  p.mt = mt;
  p.nt = nt;
  p.k = k;
  p.flags = flags;
  (void)hipEventCreate(&p.a);
  (void)hipEventCreate(&p.b);
  p.kind = kind;
  p.flops = flops;
  p.s = s;
  p.masked = e->aux_shared && s == e->aux[2];
  (void)hipEventRecord(p.a, s);
  e->evs.push_back(p);
}
void ev_end(gmb_engine* e) {
  if (!e->profiling) return;
  (void)hipEventRecord(e->evs.back().b, e->evs.back().s);
}
void ev_collect(gmb_engine* e) {  // stream already synchronised
  static FILE* trace = nullptr;
  if (!trace && !e->evs.empty()) {
    const char* path = getenv("GMB_TRACE_FILE");  // per-launch log for tuning: kind mt nt k flags ms GF
    if (path && path[0]) trace = fopen(path, "a");
  }
  // Wall time during which at least one GEMM launch of this call was in flight (union of the launch
  // intervals on the device timeline): launches of the two streams of the look-ahead schedules
  // overlap, so the SUM of their durations exceeds the time they cover.
  if (!e->evs.empty()) {
    auto interval_union = [&](auto pick) {
      std::vector<std::pair<float, float>> iv;
      for (auto& p : e->evs)
        if (pick(p.kind)) {
          float ta = 0.f, tb = 0.f;
          if (hipEventElapsedTime(&ta, e->evs[0].a, p.a) == hipSuccess && hipEventElapsedTime(&tb, e->evs[0].a, p.b) == hipSuccess)
            iv.emplace_back(ta, tb);
        }
      std::sort(iv.begin(), iv.end());
      float cur_lo = 0.f, cur_hi = -1.f;
      double uni = 0.0;
      for (auto& x : iv) {
        if (cur_hi < cur_lo || x.first > cur_hi) {
          if (cur_hi >= cur_lo) uni += cur_hi - cur_lo;
          cur_lo = x.first;
          cur_hi = x.second;
        } else if (x.second > cur_hi) {
          cur_hi = x.second;
        }
      }
      if (cur_hi >= cur_lo) uni += cur_hi - cur_lo;
      return uni;
    };
    e->tm.total_gemm_wall_ms += interval_union([](EvKind k) {
      return k == EV_CHOL_PANEL_GEMM || k == EV_CHOL_UPDATE || k == EV_CHOL_TILES_PANEL || k == EV_CHOL_SOLVE_GEMM || k == EV_PREDICT_GEMM ||
             k == EV_GRAD_GEMM;
    });
    e->tm.total_chol_gemm_wall_ms += interval_union([](EvKind k) { return k == EV_CHOL_UPDATE; });
  }
  for (auto& p : e->evs) {
    float t = 0.f;
    (void)hipEventElapsedTime(&t, p.a, p.b);
    if (trace) fprintf(trace, "%d %d %d %d %d %.5f %.1f\n", (int)p.kind, p.mt, p.nt, p.k, p.flags, t, p.flops / 1e9);
    if (p.kind != EV_LEAF && p.kind != EV_CHOL_STRIP && p.kind != EV_SOLVE_STRIP && !ev_trace_only(p.kind)) {  // every product and persistent launch
      e->tm.total_gemm_ms += t;
      e->tm.total_gemm_flops += p.flops;
      e->tm.total_gemm_launches += 1;
      if (p.masked) {
        e->tm.masked_gemm_ms += t;
        e->tm.masked_gemm_flops += p.flops;
      }
    }
    switch (p.kind) {
      case EV_CHOL_TILES:  // the persistent tile kernel: contraction, leaves and strip solves of the whole factorisation in one launch
        e->tm.total_chol_tile_ms += t;
        e->tm.total_chol_tile_flops += p.flops;
        e->tm.total_chol_tile_launches += 1;
        e->tm.chol_gemm_ms += t;
        e->tm.chol_gemm_flops += p.flops;
        e->tm.chol_gemm_launches += 1;
        break;
      case EV_EVAL_TILES:  // the persistent evaluation launch: (factorisation +) inverse + Sigma^-1 (flags & 1: with the factorisation)
        e->tm.total_eval_tile_ms += t;
        e->tm.total_eval_tile_flops += p.flops;
        e->tm.total_eval_tile_launches += 1;
        e->tm.grad_gemm_ms += t;
        e->tm.grad_gemm_flops += p.flops;
        break;
      case EV_CHOL_TILES_PANEL:  // a panel of the recursion's bottom on the tile kernel: in-panel work of the chain, like kind 0
        e->tm.chol_gemm_ms += t;
        e->tm.chol_gemm_flops += p.flops;
        e->tm.chol_gemm_launches += 1;
        e->tm.total_chol_panel_gemm_ms += t;
        e->tm.total_chol_panel_gemm_flops += p.flops;
        e->tm.total_chol_panel_tile_ms += t;
        e->tm.total_chol_panel_tile_flops += p.flops;
        e->tm.total_chol_panel_tile_launches += 1;
        break;
      case EV_CHOL_PANEL_GEMM:
      case EV_CHOL_UPDATE:
        e->tm.chol_gemm_ms += t;
        e->tm.chol_gemm_flops += p.flops;
        e->tm.chol_gemm_launches += 1;
        if (p.flags & (1 << 16)) {
          e->tm.total_chol_update_all_ms += t;
          e->tm.total_chol_update_all_flops += p.flops;
          e->tm.total_chol_update_all_launches += 1;
        }
        if (p.kind == EV_CHOL_UPDATE) {
          e->tm.total_chol_gemm_ms += t;
          e->tm.total_chol_gemm_flops += p.flops;
          e->tm.total_chol_gemm_launches += 1;
        } else {
          e->tm.total_chol_panel_gemm_ms += t;
          e->tm.total_chol_panel_gemm_flops += p.flops;
        }
        break;
      case EV_LEAF: e->tm.chol_leaf_ms += t; break;
      case EV_CHOL_SOLVE_GEMM:
      case EV_CHOL_STRIP: e->tm.chol_trsm_ms += t; break;
      case EV_PREDICT_GEMM:
        e->tm.predict_gemm_ms += t;
        e->tm.predict_gemm_flops += p.flops;
        e->tm.predict_gemm_launches += 1;
        break;
      case EV_GRAD_GEMM:
        e->tm.grad_gemm_ms += t;
        e->tm.grad_gemm_flops += p.flops;
        break;
      case EV_SOLVE_STRIP: break;
      case EV_PREDICT_COV:
      case EV_PREDICT_GRAD:
      case EV_PREDICT_GRAD_ALPHA:
      case EV_PREDICT_VGRAD:
      case EV_PREDICT_VGRAD_SOLVE:
      case EV_SPLITK:
      case EV_TERM_GRAM:
      case EV_GROUP_COV:
      case EV_SLOPE_COV:
      case EV_DESIGN:
      case EV_FITC:
      case EV_LAPLACE:
      case EV_PATHS:
      case EV_BATCH: break;
    }
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  e->evs.clear();
  if (trace) fflush(trace);
}

// ---- kernel launch helpers ----------------------------------------------------------------
// `g_in` describes the product in 128-tile units (mt, nt) and elements (k); pick the block tile so
// that the launch fills the chip, convert, schedule and launch.
long long gemm_nact128(const GemmArgs& g) {
  long long nact = 0;
  const int stride = g.nblk_stride < 1 ? 1 : g.nblk_stride;
  for (int tm = 0; tm < g.mt; ++tm) {
    int f = g.tri ? gemm_first_tn((int64_t)tm * TILE - g.tri_off - (TILE - 1), TILE, stride) : 0;
    f = f > g.nt ? g.nt : f;
    nact += g.nt - f;
  }
  return nact;
}

// The test door's pins (gmb_blk_gemm_ex): every field -1 = decide as always.  A pinned combination that launch_gemm could not
// arrive at by itself under any engine setting is refused (GMB_EINVAL) before anything is launched.  `launched` receives what ran:
//   bits 0-1 tile shape (variant) | bit 2 LDS-DMA staging | bit 3 PFC | bit 4 in place | bits 5-6 order | bits 8-15 strip |
//   bits 16-30 grid size (saturating at 0x7fff)
struct GemmPin {
  int variant = -1, staging = -1, pfc = -1, order = -1, strip = -1;
  int32_t* launched = nullptr;
};

int launch_gemm(gmb_engine* e, hipStream_t s, const GemmArgs& g_in, EvKind ev_kind, const GemmPin* pin = nullptr) {
  if (pin && pin->launched) *pin->launched = 0;
  if (g_in.mt <= 0 || g_in.nt <= 0 || g_in.k <= 0) return GMB_OK;
  GemmArgs g = g_in;
  // tiles the 128 x 128 tiling would compute
  if (g.nblk_stride < 1) g.nblk_stride = 1;
  const long long nact = gemm_nact128(g);
  const bool in_place = (const double*)g.C == g.B;  // the block must own every column of its rows
  // variant: 0 = 128x128, 1 = 64x64, 2 = 128x64, 3 = 128x32 (all 4 waves, two workgroups per compute unit)
  int variant = e->gemm_variant;
  {
    // Tile shape by a small model: a launch of T tiles on S workgroup slots (two per compute
    // unit for every shape) takes max(1, T / S + 1/2) tile times -- full rounds plus an expected
    // half round of tail -- and a tile time is tile flops / intrinsic rate.  Intrinsic rates
    // measured on MI355X on large plain products (TF/s, r02 kernels with the interleaved staging):
    // 128x128 73, 64x64 63, 128x64 65, 128x32 60.  Measured launch by launch on the N = 10k fit
    // (round 1): always-128x128 61.7 ms, always-64x64 52.2 ms, best shape
    // per launch 51.0 ms.
    static const double rate[4] = {73.0, 63.0, 65.0, 60.0};
    static const int per128[4] = {1, 4, 2, 4};  // tiles per 128 x 128 block
    const double slots = (double)e->wg_slots;
    auto score = [&](int v) {  // higher is better: 1 / predicted time
      const double t = (double)(nact * per128[v]);
      const double rounds = std::max(1.0, t / slots + 0.5);
      return rate[v] * per128[v] / rounds;
    };
    if (in_place) {
      if (g.mt != 1) return fail(e, GMB_EINVAL, "internal: in-place GEMM needs m == 128");
      variant = 0;
      if (score(2) > score(variant)) variant = 2;
      if (score(3) > score(variant)) variant = 3;
      if (pin && pin->variant >= 0) {
        if (pin->variant != 0 && pin->variant != 2 && pin->variant != 3) return fail(e, GMB_EINVAL, "gemm pin: the in-place form runs on the 128-row tiles (variants 0, 2, 3)");
        variant = pin->variant;
      }
    } else if (pin && pin->variant >= 0) {
      if (pin->variant > 3) return fail(e, GMB_EINVAL, "gemm pin: variant %d", pin->variant);
      variant = pin->variant;
    } else if (!e->force_variant) {
      variant = 0;
      if (e->small_tiles) {
        if (score(2) > score(variant)) variant = 2;
        if (score(1) > score(variant)) variant = 1;
      }
    }
  }
#ifdef GMB_TUNING
  // A/B only: variant 4 = a 256 x 128 macro-tile, eight waves (4 x 2), ONE workgroup per compute
  // unit -- the same two waves per SIMD, half the B-panel traffic per flop; m-tile counts must be even
  if (e->force_variant && e->gemm_variant == 4 && !in_place) variant = (g_in.mt % 2 == 0) ? 4 : 0;
#endif
  static const int BMs[5] = {128, 64, 128, 128, 256}, BNs[5] = {128, 64, 64, 32, 128};
  const int bm = BMs[variant], bn = BNs[variant];
  g.mt = g_in.mt * TILE / bm;
  g.nt = g_in.nt * TILE / bn;
  // triangular operand: dispatch the longest contractions first (see GemmArgs::order)
  // ... unless the launch is so large that a late long tile is a per cent of it at worst, and the L2-aware strips below -- which
  // the longest-first order gives up -- are worth more (round 6, one box, N = 50k: evaluation 1788 -> 1771 ms with the strips for
  // every product of more than lpt_max_tiles tiles; tools/gpu_grad_order_ab.py)
  g.order = 0;
  if (e->lpt_order && nact <= e->lpt_max_tiles && g.nblk_stride == 1 && g.tri_off >= 0 && !g.klo_m && (g.klo_n != 0) != (g.khi_n != 0))
    g.order = g.klo_n ? 1 : 2;
  if (pin && pin->order >= 0) {  // 1 / 2 only where the rule above could choose them, whatever the engine's settings
    const bool lpt_ok = g.nblk_stride == 1 && g.tri_off >= 0 && !g.klo_m && (g.klo_n != 0) != (g.khi_n != 0);
    if (pin->order > 2 || (pin->order != 0 && (!lpt_ok || pin->order != (g.klo_n ? 1 : 2))))
      return fail(e, GMB_EINVAL, "gemm pin: order %d is not one launch_gemm chooses for this product", pin->order);
    g.order = pin->order;
  }
  // L2-aware rasterisation of the XCD runs for launches that are several patches large (GemmArgs::strip)
  g.strip = (g.order == 0 && e->tile_strip > 0 && g.mt >= 2 && !in_place && !g.klo_m) ? e->tile_strip : 0;
  if (pin && pin->strip >= 0) {
    if (pin->strip > 255 || (pin->strip > 0 && !(g.order == 0 && g.mt >= 2 && !in_place && !g.klo_m)))
      return fail(e, GMB_EINVAL, "gemm pin: strip %d is not one launch_gemm chooses for this product", pin->strip);
    g.strip = pin->strip;
  }
  bool pfc = g.beta != 0.0 && g.k <= 1024 && !in_place;
  bool dma = e->gemm_dma && variant == 0 && !in_place;
  if (pin && pin->pfc >= 0) {  // (a pinned PFC may sit on either side of the rule's k <= 1024: a speed threshold, not a limit of the kernel)
    if (pin->pfc > 1 || (pin->pfc == 1 && (g.beta == 0.0 || in_place || variant == 0)))
      return fail(e, GMB_EINVAL, "gemm pin: C prefetch needs beta != 0, an out-of-place product and a small tile");
    pfc = pin->pfc == 1;
  }
  if (pin && pin->staging >= 0) {
    if (pin->staging > 1 || (pin->staging == 1 && (variant != 0 || in_place)))
      return fail(e, GMB_EINVAL, "gemm pin: LDS-DMA staging exists for the out-of-place 128 x 128 tile only");
    dma = pin->staging == 1;
  }
  double flops = 0.0;
  const int nblocks = gemm_schedule(g, bm, bn, &flops);
  if (nblocks <= 0) return GMB_OK;
  // Population 7 = the Cholesky's BULK trailing updates = the kind-7 launches that run the 128 x 128 kernel; they go through an
  // entry point of their own (gemm_f64_dma_chol_update_kernel, the same body), so that a rocprofv3 kernel trace lists exactly
  // the launches the live events of `roofline` time.  Kind-7 launches small enough for another tile shape count as in-panel
  // products (kind 0), like the panels' own.
  const bool bulk_update = ev_kind == EV_CHOL_UPDATE && variant == 0 && !in_place;
  const int was_update = ev_kind == EV_CHOL_UPDATE ? (1 << 16) : 0;  // issued AS a trailing update, whatever tile shape it runs (total_chol_update_all_*)
  if (ev_kind == EV_CHOL_UPDATE && !bulk_update) ev_kind = EV_CHOL_PANEL_GEMM;
  ev_begin(e, s, ev_kind, flops, g_in.mt, g_in.nt, g.k,
           g.tri | (g.klo_n << 3) | (g.khi_n << 4) | (g.klo_m << 5) | (variant << 8) | was_update);
  const dim3 grid(nblocks);
  if (pin && pin->launched)
    *pin->launched = variant | (dma ? 4 : 0) | (variant != 0 && pfc ? 8 : 0) | (in_place ? 16 : 0) | (g.order << 5) | ((g.strip & 0xff) << 8) |
                     (std::min(nblocks, 0x7fff) << 16);
  switch (variant) {
    case 0:
      if (dma && bulk_update) hipLaunchKernelGGL(gemm_f64_dma_chol_update_kernel, grid, dim3(256), 0, s, g);
      else if (dma) hipLaunchKernelGGL(gemm_f64_dma_kernel, grid, dim3(256), 0, s, g);
      else hipLaunchKernelGGL((gemm_f64_kernel<2, 2, 4, 4, 2>), grid, dim3(256), 0, s, g);
      break;
#ifdef GMB_TUNING
    case 4: hipLaunchKernelGGL((gemm_f64_kernel<4, 2, 4, 4, 1>), grid, dim3(512), 0, s, g); break;
#endif
    // small tiles with a short contraction and beta != 0: the C-prefetching instantiations (gemm_f64.hpp)
    case 1:
      if (pfc) hipLaunchKernelGGL((gemm_f64_kernel<2, 2, 2, 2, 2, true>), grid, dim3(256), 0, s, g);
      else hipLaunchKernelGGL((gemm_f64_kernel<2, 2, 2, 2, 2>), grid, dim3(256), 0, s, g);
      break;
    case 2:
      if (pfc) hipLaunchKernelGGL((gemm_f64_kernel<2, 2, 4, 2, 2, true>), grid, dim3(256), 0, s, g);
      else hipLaunchKernelGGL((gemm_f64_kernel<2, 2, 4, 2, 2>), grid, dim3(256), 0, s, g);
      break;
    default:
      if (pfc) hipLaunchKernelGGL((gemm_f64_kernel<2, 2, 4, 1, 2, true>), grid, dim3(256), 0, s, g);
      else hipLaunchKernelGGL((gemm_f64_kernel<2, 2, 4, 1, 2>), grid, dim3(256), 0, s, g);
      break;
  }
  ev_end(e);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// B <- B inv(L_kk)^T on `nrows` rows (multiple of 16): one wavefront per 16 rows
int launch_trsm_strip(gmb_engine* e, hipStream_t s, double* B, int64_t ldb, int64_t nrows, const double* L, int64_t ldl,
                      const double* dinv16, int nvalid, EvKind ev_kind) {
  if (nrows <= 0) return GMB_OK;
  TrsmArgs t;
  t.B = B;
  t.ldb = ldb;
  t.nrows = nrows;
  t.L = L;
  t.ldl = ldl;
  t.dinv16 = dinv16;
  t.nvalid = nvalid;
  ev_begin(e, s, ev_kind, (double)nrows * TILE * TILE);
  hipLaunchKernelGGL(trsm_strip_kernel, dim3((unsigned)((nrows / 16 + 3) / 4)), dim3(256), 0, s, t);
  ev_end(e);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

int launch_leaf(gmb_engine* e, hipStream_t s, const LeafArgs& a) {
  ev_begin(e, s, EV_LEAF, 0.0);
  if (e->naive_leaf)
    hipLaunchKernelGGL(potrf_leaf_naive_kernel, dim3(1), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(potrf_leaf_kernel, dim3(1), dim3(512), 0, s, a);
  ev_end(e);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// grid = the strips of cov_tile_kernel's enumeration (strip tiles per workgroup along the column index)
long long cov_grid_blocks(int ti, int tj, int strip, int tri_grid, int row_first, int row_stride) {
  const int S = strip < 1 ? 1 : strip;
  const long long nst = (tj + S - 1) / S;
  if (row_stride > 0) return row_first < ti ? ((ti - 1 - row_first) / row_stride + 1) * nst : 0;
  if (tri_grid) return cov_tri_blocks_before(ti, tj, S);
  return (long long)ti * nst;
}

int launch_cov(gmb_engine* e, const CovTileArgs& a_in) {
  if (a_in.ti <= 0 || a_in.tj <= 0) return GMB_OK;
  CovTileArgs a = a_in;
  const double tiles = (double)a.ti * a.tj * (a.lower_only ? 0.5 : 1.0) / (a.row_stride > 0 ? a.row_stride : 1);  // this launch's share
  a.stream_stores = tiles * TILE * TILE * 8.0 >= 1073741824.0 / (a.row_stride > 0 ? a.row_stride : 1);  // by the whole matrix
  // tiles per workgroup: enough strips left to fill the chip's ~800 workgroup slots several times over
  a.strip = e->cov_strip > 0 ? e->cov_strip : (tiles >= 32768.0 ? 4 : tiles >= 12288.0 ? 2 : 1);
  // small grids (up to 1024 tiles, N <= 5.7k): four workgroups per tile (N = 392: the build's one launch 29.6 -> 11.8 us, N = 2560:
  // 43 -> 30, N = 4000: 55 -> 39, N = 5200: 61 -> 50; from ~2000 tiles on the split costs more than the direct-loop tiles' tail)
  a.gsplit = (a.strip == 1 && cov_grid_blocks(a.ti, a.tj, 1, a.tri_grid, a.row_first, a.row_stride) <= 1024) ? 4 : 1;
  const long long nb = cov_grid_blocks(a.ti, a.tj, a.strip, a.tri_grid, a.row_first, a.row_stride) * (a.gsplit > 1 ? a.gsplit : 1);
  if (nb <= 0) return GMB_OK;
  const dim3 grid((unsigned)nb), block(256);
  const bool known = with_kind_nc(a.p.kind, e->nc_pad, [&](auto kind, auto nc) {
    constexpr int K = decltype(kind)::value, NC = decltype(nc)::value;
    hipLaunchKernelGGL((cov_tile_kernel<K, NC>), grid, block, 0, e->stream, a);
  });
  if (!known) return fail(e, GMB_EINVAL, "unknown kernel kind %d", a.p.kind);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

int spec_ntab(const gmb_kernel_spec& s) { return s.n_coreg + (s.out_col >= 0 ? 1 : 0); }

int validate_spec(gmb_engine* e, const gmb_kernel_spec& s, int D) {
  if (s.kind < 0 || s.kind > 4) return fail(e, GMB_EINVAL, "kernel kind %d out of range", s.kind);
  if (s.n_cont < 1 || s.n_cont > GMB_MAX_DIMS)
    return fail(e, GMB_EINVAL, "n_cont=%d must be in [1,%d]", s.n_cont, GMB_MAX_DIMS);
  if (s.n_lin < 0 || s.n_lin > GMB_MAX_LIN)
    return fail(e, GMB_EINVAL, "n_lin=%d must be in [0,%d]", s.n_lin, GMB_MAX_LIN);
  if (s.n_coreg < 0 || s.n_coreg > GMB_MAX_COREG)
    return fail(e, GMB_EINVAL, "bad n_coreg=%d", s.n_coreg);
  for (int k = 0; k < s.n_cont; ++k)
    if (s.idx_cont[k] < 0 || (D > 0 && s.idx_cont[k] >= D))
      return fail(e, GMB_EINVAL, "idx_cont[%d]=%d outside the %d columns of X", k, s.idx_cont[k], D);
  for (int k = 0; k < s.n_lin; ++k)
    if (s.idx_lin[k] < 0 || (D > 0 && s.idx_lin[k] >= D))
      return fail(e, GMB_EINVAL, "idx_lin[%d]=%d outside the %d columns of X", k, s.idx_lin[k], D);
  for (int t = 0; t < s.n_coreg; ++t) {
    if (s.coreg_col[t] < 0 || (D > 0 && s.coreg_col[t] >= D))
      return fail(e, GMB_EINVAL, "coreg_col[%d]=%d outside X", t, s.coreg_col[t]);
    if (s.coreg_levels[t] < 1 || s.coreg_levels[t] > GMB_MAX_LEVELS)
      return fail(e, GMB_EINVAL, "coreg_levels[%d]=%d must be in [1,%d]", t, s.coreg_levels[t],
                  GMB_MAX_LEVELS);
  }
  if (s.out_col >= 0) {
    if (D > 0 && s.out_col >= D) return fail(e, GMB_EINVAL, "out_col=%d outside X", s.out_col);
    if (s.n_out < 1 || s.n_out > GMB_MAX_LEVELS)
      return fail(e, GMB_EINVAL, "n_out=%d must be in [1,%d]", s.n_out, GMB_MAX_LEVELS);
  }
  if (!(s.jitter >= 0.0)) return fail(e, GMB_EINVAL, "jitter must be >= 0");
  return GMB_OK;
}

// Fill the terms' PrepArgs / CovParams from spec + theta and upload the coregion tables.
int apply_theta(gmb_engine* e) {
  const gmb_kernel_spec& s = e->spec;
  const double* th = e->theta.data();
  int k = 0;
  const int n_ls = s.ard ? s.n_cont : 1;
  PrepArgs pa{};
  const int per = e->periodic;
  pa.nc = per ? 2 * s.n_cont : s.n_cont;
  pa.nc_pad = e->nc_pad;
  pa.periodic = per;
  // Periodic models: dimension i feeds the prepared columns 2i, 2i + 1, both with the weight w_i = 1 / ls_i (<kind>+Periodic:
  // r^2 = sum 4 sin^2(pi D / T) / ls^2) or 1 / (2 ls_i) (Periodic = ExpQuad on sum sin^2(pi D / T) / ls^2).  The halving is exact,
  // so grad_reduce gets the gradient's true 1 / ls_i back as 2 w_i.
  auto set_ls = [&](PrepArgs& p, int i, double ls) {
    if (!per) {
      p.inv_ls[i] = 1.0 / ls;
      return;
    }
    p.inv_ls[2 * i] = p.inv_ls[2 * i + 1] = per == 2 ? 0.5 * (1.0 / ls) : 1.0 / ls;
  };
  for (int i = 0; i < s.n_cont; ++i) {
    const double ls = th[s.ard ? i : 0];
    if (!(ls > 0.0)) return fail(e, GMB_EINVAL, "lengthscale %d = %g must be positive", i, ls);
    if (!per) {
      pa.idx_cont[i] = s.idx_cont[i];
    } else {
      pa.idx_cont[2 * i] = pa.idx_cont[2 * i + 1] = s.idx_cont[i];
      pa.two_over_T[i] = 2.0 / e->periods[i];
    }
    set_ls(pa, i, ls);
  }
  k += n_ls;
  const double eta = th[k], sigma = th[k + 1];
  k += 2;
  CovParams cp{};
  cp.kind = s.kind;
  cp.eta2 = eta * eta;
  cp.sigma2 = sigma * sigma;
  cp.jitter = s.jitter;
  cp.n_lin = s.n_lin;
  pa.n_lin = s.n_lin;
  if (s.n_lin > 0) {
    for (int i = 0; i < s.n_lin; ++i) {
      pa.idx_lin[i] = s.idx_lin[i];
      pa.c_lin[i] = th[k + i];
    }
    cp.tau = th[k + s.n_lin];
    k += s.n_lin + 1;
  }
  // coregion tables: B = W W^T + diag(kappa)
  const int ntab = spec_ntab(s);
  cp.n_tab = ntab;
  pa.n_tab = ntab;
  e->htabs.clear();
  int off = 0;
  for (int t = 0; t < ntab; ++t) {
    const bool is_out = (t == s.n_coreg);
    const int L = is_out ? s.n_out : s.coreg_levels[t];
    const double* W = th + k;
    const double* kap = th + k + 2 * L;
    cp.tab_levels[t] = L;
    cp.tab_off[t] = off;
    pa.tab_col[t] = is_out ? s.out_col : s.coreg_col[t];
    pa.tab_levels[t] = L;
    for (int a = 0; a < L; ++a)
      for (int b = 0; b < L; ++b)
        e->htabs.push_back(W[2 * a] * W[2 * b] + W[2 * a + 1] * W[2 * b + 1] + (a == b ? kap[a] : 0.0));
    off += L * L;
    k += 3 * L;
  }
  cp.noise_tab = -1;
  e->hnoise.clear();
  if (s.out_col >= 0 && s.hetero_noise) {
    const int P = s.n_out;
    const double* W = th + k;
    const double* kap = th + k + 2 * P;
    for (int a = 0; a < P; ++a) e->hnoise.push_back(W[2 * a] * W[2 * a] + W[2 * a + 1] * W[2 * a + 1] + kap[a]);
    cp.noise_tab = s.n_coreg;  // the output table's category index
    k += 3 * P;
  }
  // additive model: per coregion dim one more [ls | eta | (c, tau)] block (validated here, used below)
  const int k_add = k;
  if (s.additive) k += s.n_coreg * (n_ls + 1 + (s.n_lin > 0 ? s.n_lin + 1 : 0));
  if (k != (int)e->theta.size()) return fail(e, GMB_EINVAL, "internal: theta packing mismatch");
  if (!e->dtabs) {
    int rc = e->dtabs.renew(e->pool, (int64_t)MAX_TABS * GMB_MAX_LEVELS * GMB_MAX_LEVELS);
    if (rc) return rc;
    rc = e->dnoise.renew(e->pool, (int64_t)GMB_MAX_LEVELS);
    if (rc) return rc;
  }
  if (!e->htabs.empty())
    HIP_TRY(e, hipMemcpyAsync(e->dtabs, e->htabs.data(), e->htabs.size() * sizeof(double),
                              hipMemcpyHostToDevice, e->stream));
  if (!e->hnoise.empty())
    HIP_TRY(e, hipMemcpyAsync(e->dnoise, e->hnoise.data(), e->hnoise.size() * sizeof(double),
                              hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));  // host vectors may be rewritten by the caller
  cp.tabs = e->dtabs;
  cp.noise_mult = e->dnoise;
  // ---- terms ----
  e->terms.clear();
  if (!s.additive) {
    e->terms.push_back(gmb_engine::Term{pa, cp, eta, ntab});
    return GMB_OK;
  }
  const PrepArgs pa_all = pa;
  const CovParams cp_all = cp;
  auto select_tables = [&](gmb_engine::Term& t, int dim) {  // dim < 0: output table only
    int n = 0;
    auto take = [&](int src) {
      t.cp.tab_levels[n] = cp_all.tab_levels[src];
      t.cp.tab_off[n] = cp_all.tab_off[src];
      t.pa.tab_col[n] = pa_all.tab_col[src];
      t.pa.tab_levels[n] = pa_all.tab_levels[src];
      ++n;
    };
    if (dim >= 0) take(dim);
    if (s.out_col >= 0) take(s.n_coreg);
    t.cp.n_tab = t.pa.n_tab = t.n_tab_acc = n;
    t.cp.noise_tab = (dim < 0 && s.out_col >= 0 && s.hetero_noise) ? n - 1 : -1;
  };
  gmb_engine::Term t0{pa_all, cp_all, eta, 0};
  select_tables(t0, -1);
  e->terms.push_back(t0);
  int ka = k_add;
  for (int j = 0; j < s.n_coreg; ++j) {
    gmb_engine::Term t{pa_all, cp_all, 0.0, 0};
    for (int i = 0; i < s.n_cont; ++i) {
      const double ls = th[ka + (s.ard ? i : 0)];
      if (!(ls > 0.0)) return fail(e, GMB_EINVAL, "lengthscale %d of additive term %d = %g must be positive", i, j, ls);
      set_ls(t.pa, i, ls);  // (periodic: the term's own lengthscales on the shared periods)
    }
    ka += n_ls;
    t.eta = th[ka++];
    t.cp.eta2 = t.eta * t.eta;
    if (s.n_lin > 0) {
      for (int i = 0; i < s.n_lin; ++i) t.pa.c_lin[i] = th[ka + i];
      t.cp.tau = th[ka + s.n_lin];
      ka += s.n_lin + 1;
    }
    t.cp.sigma2 = 0.0;  // the noise is written by the first pass only
    t.cp.jitter = 0.0;
    select_tables(t, j);
    e->terms.push_back(t);
  }
  return GMB_OK;
}

// what ONE preparation launch clears besides its own work: 64-bit words at two addresses (PrepArgs::zero).  Default: nothing.
struct PrepClears {
  unsigned long long* p[2] = {nullptr, nullptr};
  int64_t words[2] = {0, 0};
};

PrepArgs prep_args(gmb_engine* e, const double* dXraw, int64_t n, int64_t ldx, int64_t npad, double* xs, double* xl, int32_t* cat,
                   const PrepArgs* proto, const PrepClears& clears = PrepClears{}) {
  PrepArgs a = proto ? *proto : e->terms[0].pa;  // (every caller sits behind gmb_set_theta's apply_theta: terms is not empty)
  for (int z = 0; z < 2; ++z) {
    a.zero[z] = clears.p[z];
    a.zero_words[z] = clears.words[z];
  }
  a.X = dXraw;
  a.n = n;
  a.ldx = ldx;
  a.npad = npad;
  a.xs = xs;
  a.xl = xl;
  a.cat = cat;
  return a;
}

int prep_points(gmb_engine* e, const double* dXraw, int64_t n, int64_t ldx, int64_t npad, double* xs,
                double* xl, int32_t* cat, const PrepArgs* proto = nullptr, const PrepClears& clears = PrepClears{}) {
  const PrepArgs a = prep_args(e, dXraw, n, ldx, npad, xs, xl, cat, proto, clears);
  hipLaunchKernelGGL(prep_points_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, e->stream, a);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// N (hence Np, Nr, ld) changes -- gmb_set_data, resize_n: every workspace whose size or layout follows from them is stale, and
// so is the cached launch plan of the triangular inverse.  The union of what the two sites used to mark, one line each.  (The
// prepared points (pts) were marked by gmb_set_data only and stay there: resize_n keeps them when they are large enough.)
void stale_sized_by_n(gmb_engine* e) {
  e->pw.stale();
  e->tg.stale();
  e->pw2.stale();
  e->dpart.stale();
  e->pg.stale();
  e->ga.stale();
  e->slope.stale();
  e->dz.stale();
  e->plan_N = -1;
}

PointSet train_set(const gmb_engine* e) { return PointSet{e->pts.xs, e->pts.xl, e->pts.cat, e->N, e->Nr}; }

// the full factor buffer (Nr x Np, leading dimension Nr), allocated on first use
int ensure_factor_buffer(gmb_engine* e) { return e->dA.reserve(e->pool, e->ld * e->Np); }

// the training factor as the Cholesky / triangular-solve routines take it
FactorRef train_factor(gmb_engine* e) { return FactorRef{e->dA, e->ld, e->N, e->Np, e->Nr, e->dDinv16, e->dscal, &e->dct}; }

// The walk over the model's covariance terms (term_walk.hpp): body(t) runs with the resident training points prepared for term t.
// This is the ONE place they are re-prepared for a term, and term 0's preparation is back when the walk returns, however it ends.
// Test points are a body's own business (workspace, not engine state).
// `mask` selects the terms visited (bit t = terms[t]); a selection is an argument of the call that makes it, never engine state.
template <typename Body>
int walk_terms(gmb_engine* e, uint32_t mask, Body&& body) {
  return for_each_term(
      (int)e->terms.size(), mask,
      [e](int t) { return prep_points(e, e->dX, e->N, e->D, e->Nr, e->pts.xs, e->pts.xl, e->pts.cat, &e->terms[t].pa); }, body);
}

// ... every term: what all train-side builds walk
template <typename Body>
int walk_terms(gmb_engine* e, Body&& body) {
  return walk_terms(e, ALL_TERMS, body);
}

// all bits of a model's selection mask (at most 1 + GMB_MAX_COREG terms)
uint32_t all_terms_mask(const gmb_engine* e) { return (1u << e->terms.size()) - 1u; }

// Term t's parameters for the pass that STORES (the first selected term): noise and jitter belong to no term and ride on that
// pass, whichever term it is.  sigma2, the noise table and the jitter are terms[0].cp's -- a later term's own cp holds none of
// them -- and the noise level is read from the OUTPUT table, which every term's preparation carries last.
CovParams first_pass_params(const gmb_engine* e, int t) {
  if (t == 0) return e->terms[0].cp;
  CovParams p = e->terms[t].cp;
  const CovParams& p0 = e->terms[0].cp;
  p.sigma2 = p0.sigma2;
  p.jitter = p0.jitter;
  p.noise_mult = p0.noise_mult;
  p.noise_tab = p0.noise_tab >= 0 ? p.n_tab - 1 : -1;
  return p;
}

// What every train x train build of Sigma passes the covariance launch: `out` (leading dimension ldo) takes ti x tj tiles of the
// lower triangle, y row and identity padding included.  The caller adds what is its own (the grid, the block rows it owns).
CovTileArgs train_cov_args(gmb_engine* e, double* out, int64_t ldo, int ti, int tj) {
  CovTileArgs a{};
  a.p = e->terms[0].cp;
  a.rows = a.cols = train_set(e);
  a.out = out;
  a.ldo = ldo;
  a.ti = ti;
  a.tj = tj;
  a.mode = COV_TRAIN;
  a.lower_only = 1;
  a.y = e->dy;
  return a;
}

// ... and the build itself: term 0 writes, an additive model's further terms add their covariance to the real entries
int launch_train_cov(gmb_engine* e, CovTileArgs& a) {
  return walk_terms(e, [&](int t) {
    a.p = e->terms[t].cp;
    a.accumulate = t > 0;
    return launch_cov(e, a);
  });
}

// Covariance build: lower-triangular tiles of Sigma = K + noise + jitter, the y row, identity padding, written
// column-major into `out` (Nr x Np, leading dimension ldo) -- the factor buffer in gmb_factorize.  `inline_prep`, if given (a small
// gmb_evaluate, EvalPlan::inline_prep): this launch prepares the points it stages, and clears what prep_points_kernel would have.
int build_sigma(gmb_engine* e, double* out, int64_t ldo, const PrepClears* inline_prep = nullptr) {
  CovTileArgs a = train_cov_args(e, out, ldo, (int)(e->Nr / TILE), (int)(e->Np / TILE));
  a.tri_grid = 1;
  if (inline_prep) {
    a.inline_prep = 1;
    a.prep = prep_args(e, e->dX, e->N, e->D, e->Nr, e->pts.xs, e->pts.xl, e->pts.cat, nullptr, *inline_prep);
  }
  return launch_train_cov(e, a);
}

// ---- Cholesky recursion -------------------------------------------------------------------
// `rend`: block row where the panel solve / updates stop (the whole matrix, or the end of a
// diagonal square when the rows below are solved later in bulk)
int chol_leaf(gmb_engine* e, hipStream_t s, const FactorRef& f, int c, int rend) {
  LeafArgs a{};
  a.A = f.A + (int64_t)c * TILE + (int64_t)c * TILE * f.ld;
  a.lda = f.ld;
  a.nvalid = (int)std::min<int64_t>(TILE, f.N - (int64_t)c * TILE);
  a.dinv16 = f.dinv16 + (int64_t)c * 8 * 256;
  a.logdet = f.scal;
  a.info = f.info();
  a.row0 = (int64_t)c * TILE;
  a.dbg = nullptr;
  int rc = launch_leaf(e, s, a);
  if (rc) return rc;
  // panel rows below the diagonal block:  P <- P inv(L_cc)^T   (in place, 16 rows per wavefront)
  return launch_trsm_strip(e, s, f.A + (int64_t)(c + 1) * TILE + (int64_t)c * TILE * f.ld, f.ld,
                           (int64_t)(rend - c - 1) * TILE, a.A, f.ld, a.dinv16, a.nvalid, EV_CHOL_STRIP);
}

int chol_tiles_panel(gmb_engine* e, hipStream_t s, const FactorRef& f, int c0, int c1, int rend, CholResult* res);

// `update_kind`: what the trailing updates are timed as -- EV_CHOL_UPDATE (bulk) for the plain recursion over the whole matrix,
// EV_CHOL_PANEL_GEMM (in-panel product of the latency-bound chain) inside the look-ahead schedules' panels.  `tile_panels`, if
// given: panels of <= panel_tiles_w block columns go to the tile kernel (chol_tiles_panel), which reports there.
int chol_cols(gmb_engine* e, hipStream_t s, const FactorRef& f, int c0, int c1, int rend, EvKind update_kind, CholResult* tile_panels = nullptr) {
  if (c1 - c0 == 1) return chol_leaf(e, s, f, c0, rend);
  if (tile_panels && c1 - c0 <= e->panel_tiles_w) return chol_tiles_panel(e, s, f, c0, c1, rend, tile_panels);
  const int mid = c0 + (c1 - c0 + 1) / 2;
  int rc = chol_cols(e, s, f, c0, mid, rend, update_kind, tile_panels);
  if (rc) return rc;
  GemmArgs g{};
  g.C = f.A + (int64_t)mid * TILE + (int64_t)mid * TILE * f.ld;
  g.ldc = f.ld;
  g.A = f.A + (int64_t)mid * TILE + (int64_t)c0 * TILE * f.ld;
  g.lda = f.ld;
  g.B = g.A;
  g.ldb = f.ld;
  g.mt = c1 - mid;
  g.nt = rend - mid;
  g.k = (mid - c0) * TILE;
  g.alpha = -1.0;
  g.beta = 1.0;
  g.tri = 1;
  rc = launch_gemm(e, s, g, update_kind);
  if (rc) return rc;
  return chol_cols(e, s, f, mid, c1, rend, update_kind, tile_panels);
}

// The ragged last block of the persistent launches (chol_tiles.hpp: ct_ksum<.., RAG>): the fraction of a tile's contraction that
// the last block ROW's tasks (rows: the y row included) and the last block COLUMN's solve / inverse tasks still perform
double ragged_row_frac(const FactorRef& f) {
  const int64_t rv = f.N + 1 - (f.Nr - TILE);
  return rv >= TILE ? 1.0 : (double)((rv + 15) / 16) / 8.0;
}
double ragged_col_frac(const FactorRef& f) {
  const int64_t cv = f.N - (f.Np - TILE);
  return cv >= TILE ? 1.0 : (double)((cv + 15) / 16) / 8.0;
}
// flops of the tile Cholesky's contractions (2 * 128^3 per k-block of a tile) on nct block columns with the nrt block rows from
// their diagonal down; the last block row of the bordered matrix contracts its real rows only
double chol_tiles_flops(const FactorRef& f, int nct, int nrt, bool to_last_row = true) {
  const double fr = to_last_row ? ragged_row_frac(f) : 1.0;
  double flops = 0.0;
  for (int j = 1; j < nct; ++j) {
    const double tiles = nrt - 1 > j ? (double)(nrt - j - 1) + fr : (double)(nrt - j);  // (the diagonal tile is never cut)
    flops += 2.0 * TILE * TILE * TILE * (double)j * tiles;
  }
  return flops;
}

// ---- persistent tile Cholesky (chol_tiles.hpp): the whole factorisation in one launch --------------------
// What every persistent launch passes alike: block columns [c0, c0 + nct) of f from their diagonal down, the control words at
// the head of f's control block (sized by the caller) with the tile flags behind them.  `chol`: the launch factors -- log-det,
// info word and the chain words behind nrt x nct tile flags.
CholTilesArgs tiles_args(const FactorRef& f, int c0, int nct, int nrt, int ntasks, bool chol = true) {
  uint32_t* ct = *f.ct;
  CholTilesArgs a{};
  a.A = f.A + (int64_t)c0 * TILE * (f.ld + 1);
  a.ld = f.ld;
  a.nct = nct;
  a.nrt = nrt;
  a.N = f.N - (int64_t)c0 * TILE;
  a.row_base = (int64_t)c0 * TILE;
  a.dinv16 = f.dinv16 + (int64_t)c0 * 8 * 256;
  a.ctl = ct;
  a.flags = ct + 4;
  if (chol) {
    a.logdet = f.scal;
    a.info = f.info();
    a.half = ct + 4 + (int64_t)nrt * nct;
    a.prog = a.half + 2 * (int64_t)nct;
  }
  a.ntasks = ntasks;
  a.timeout_us = 4000000u;  // a wait of 4 s means a lost flag: give the launch up, never the GPU
  return a;
}

// fault injection (gmb_debug_chol_lose_tickets): tickets 0 .. lose-1 of the launch behind the cleared control block are never
// handed out
int tiles_lose_tickets(gmb_engine* e, hipStream_t s, uint32_t* ctl, int lose) {
  const uint32_t first = (uint32_t)lose;
  HIP_TRY(e, hipMemcpyAsync(ctl, &first, sizeof first, hipMemcpyHostToDevice, s));
  HIP_TRY(e, hipStreamSynchronize(s));  // (`first` lives on this stack frame)
  return GMB_OK;
}

// a traced launch stamps its tasks into the engine's trace buffer (gmb_chol_task_trace), cleared here
int tiles_trace_buffer(gmb_engine* e, hipStream_t s, CholTilesArgs& a) {
  int rc;
  if ((rc = e->dct_trace.reserve(e->pool, 4 * (int64_t)a.ntasks))) return rc;
  HIP_TRY(e, hipMemsetAsync(e->dct_trace, 0, (size_t)a.ntasks * 4 * sizeof(unsigned long long), s));
  a.dbg = e->dct_trace;
  return GMB_OK;
}

// `trace`, `lose`: task stamps and injected faults, as the caller of the factorisation asks for them
int chol_tiles(gmb_engine* e, hipStream_t s, const FactorRef& f, bool trace, int lose, CholResult* res) {
  const int nct = (int)(f.Np / TILE), nrt = (int)(f.Nr / TILE);
  const int ntasks = ct_task_count(nct, nrt);
  const int64_t words = 4 + (int64_t)nrt * nct + 3 * (int64_t)nct;
  int rc;
  if ((rc = f.ct->reserve(e->pool, words))) return rc;
  HIP_TRY(e, hipMemsetAsync(*f.ct, 0, (size_t)words * sizeof(uint32_t), s));
  res->injected = lose > 0;
  if (lose > 0 && (rc = tiles_lose_tickets(e, s, *f.ct, lose))) return rc;
  CholTilesArgs a = tiles_args(f, 0, nct, nrt, ntasks);
  res->traced = trace;
  if (trace && (rc = tiles_trace_buffer(e, s, a))) return rc;
  const double flops = chol_tiles_flops(f, nct, nrt);
  // eight-wave workgroups, one per compute unit: every phase of the latency chain has the whole compute unit (N = 10k:
  // 6.8 ms against 8.7 ms with four-wave workgroups, two per compute unit -- which stay available to the tuning build)
  int nw = 8;
#ifdef GMB_TUNING
  if (const char* cw = getenv("GMB_CT_WAVES")) nw = atoi(cw) == 4 ? 4 : 8;
#endif
  int grid = (int)std::min<long long>(ntasks, nw == 8 ? e->wg_slots / 2 : e->wg_slots);
#ifdef GMB_TUNING
  if (const char* cg = getenv("GMB_CT_GRID")) grid = std::max(1, std::min(grid, atoi(cg)));
#endif
  ev_begin(e, s, EV_CHOL_TILES, flops, nct, nrt, (int)f.Np, 0);
  if (nw == 8) hipLaunchKernelGGL(chol_tiles_kernel<8>, dim3(grid), dim3(512), 0, s, a);
  else hipLaunchKernelGGL(chol_tiles_kernel<4>, dim3(grid), dim3(256), 0, s, a);
  ev_end(e);
  HIP_TRY(e, hipGetLastError());
  res->tiles = true;
  res->ntasks = ntasks;
  return GMB_OK;
}

// Block columns [c0, c1) of the factor with every row below them down to block row `rend`, updated by everything left of
// c0 already: ONE launch of the tile kernel on that panel (left-looking tile tasks inside it; the rows below the square ride
// along as in the whole-matrix form).  Replaces, per panel of 16 block columns at C3, 16 leaf + 16 strip + 15 product launches
// (the 64 x 64-tile products that run at 45 TF/s: profiles/r05_bench_c3_kernel_stats.csv).  The control block is the tile
// Cholesky's; its ABORT word is not cleared between the panels of one factorisation (chol_factor clears it once), so a
// panel that gave up waiting makes every later one drain and the host sees it at the end.
int chol_tiles_panel(gmb_engine* e, hipStream_t s, const FactorRef& f, int c0, int c1, int rend, CholResult* res) {
  const int nct = c1 - c0, nrt = rend - c0;
  const int ntasks = ct_task_count(nct, nrt);
  const int64_t words = 4 + (int64_t)nrt * nct + 3 * (int64_t)nct;
  int rc;
  if ((rc = f.ct->reserve(e->pool, std::max<int64_t>(words, 4 + (int64_t)(e->panel_tiles_w + 3) * (f.Nr / TILE))))) return rc;  // (one size for every panel of the matrix)
  HIP_TRY(e, hipMemsetAsync(*f.ct, 0, sizeof(uint32_t), s));                                  // the ticket counter
  HIP_TRY(e, hipMemsetAsync(*f.ct + 2, 0, (size_t)(words - 2) * sizeof(uint32_t), s));       // flags and chain words
  const CholTilesArgs a = tiles_args(f, c0, nct, nrt, ntasks);
  const double flops = chol_tiles_flops(f, nct, nrt, rend == (int)(f.Nr / TILE));
  const int grid = (int)std::min<long long>(ntasks, e->wg_slots / 2);
  ev_begin(e, s, EV_CHOL_TILES_PANEL, flops, nct, nrt, nct * TILE, 0);
  hipLaunchKernelGGL(chol_tiles_kernel<8>, dim3(grid), dim3(512), 0, s, a);
  ev_end(e);
  HIP_TRY(e, hipGetLastError());
  res->tiles = true;  // (the abort word is read back with the factorisation's scalars)
  return GMB_OK;
}

// V <- V L^-T (V: ntm x Np/128 tiles, leading dimension ldv) as one persistent launch (chol_tiles.hpp: trsm_tiles_kernel)
int trsm_tiles(gmb_engine* e, hipStream_t s, const FactorRef& f, double* V, int64_t ldv, int ntm, EvKind ev_kind, bool* launched) {
  const int nct = (int)(f.Np / TILE);
  const long long ntasks = (long long)ntm * nct;
  if (ntasks <= 0) return GMB_OK;
  const int64_t words = 4 + (int64_t)ntm * nct;
  int rc;
  if ((rc = f.ct->reserve(e->pool, words))) return rc;
  HIP_TRY(e, hipMemsetAsync(*f.ct, 0, (size_t)words * sizeof(uint32_t), s));
  CholTilesArgs a = tiles_args(f, 0, nct, nct, (int)ntasks, false);
  a.V = V;
  a.ldv = ldv;
  a.ntm = ntm;
  double flops = 0.0;
  for (int c = 0; c < nct; ++c)
    flops += (double)ntm * (2.0 * TILE * TILE * TILE * c * (c == nct - 1 ? ragged_col_frac(f) : 1.0) + (double)TILE * TILE * TILE);
  const int grid = (int)std::min<long long>(ntasks, e->wg_slots / 2);
  ev_begin(e, s, ev_kind, flops, nct, ntm, (int)f.Np, 0);
  hipLaunchKernelGGL(trsm_tiles_kernel<8>, dim3(grid), dim3(512), 0, s, a);
  ev_end(e);
  HIP_TRY(e, hipGetLastError());
  *launched = true;
  return GMB_OK;
}

// One persistent launch for L^-T (rows), Sigma^-1 = U U^T into dW and the alpha parts -- with the factorisation's own tile
// tasks in the same launch (with_chol) or behind a factorisation that is already final (eval_tiles.hpp).
int grad_workspace(gmb_engine* e);
// 32-bit words of the evaluation launch's control block:
// [4 control | nrt x nct tile flags | 3 nct chain words | nct x nct U flags | nct counts of finished INV tasks per block row]
int64_t eval_tiles_words(int nct, int nrt) { return 4 + (int64_t)nrt * nct + 3 * (int64_t)nct + (int64_t)nct * nct + nct; }

// gmb_evaluate with a gradient runs as the fused launch (what its plan's `light` rests on)
bool eval_will_fuse(const gmb_engine* e) {
  const int nblocks = (int)(e->Np / TILE);
  return !e->naive_leaf && (e->chol_scheme == 3 || e->chol_scheme < 0) && e->grad_scheme != 0 && e->grad_scheme != 1 &&
         nblocks <= e->tiles_max_blocks && (e->grad_scheme == 2 ? nblocks >= 1 : nblocks >= e->et_min_blocks);
}

// gmb_evaluate's plan (eval_plan.hpp), from the engine as it stands when the call begins -- data and kernel are set, theta need
// not be: an additive model has one term for the whole table and one per coregion dimension (apply_theta)
EvalPlan plan_evaluate_call(const gmb_engine* e, bool with_grad) {
  EvalPlanIn in;
  in.with_grad = with_grad;
  in.will_fuse = eval_will_fuse(e);
  in.ct_lose = e->ct_lose;
  in.nterms = e->spec.additive ? 1 + e->spec.n_coreg : 1;
  in.Nr = e->Nr;
  in.Np = e->Np;
  in.inline_prep_max_rows = e->inline_prep_max_rows;
  in.naive_leaf = e->naive_leaf;
  in.profiling = e->profiling;
  return plan_evaluation(in);
}

// what the preparation launch of a plan with `prezero` clears: the scalar block and the tile launch's control words (which
// set_theta has reserved by then)
PrepClears eval_clears(gmb_engine* e) {
  const int64_t words = eval_tiles_words((int)(e->Np / TILE), (int)(e->Nr / TILE));
  using U64 = unsigned long long;
  return PrepClears{{reinterpret_cast<U64*>(e->dscal.p), reinterpret_cast<U64*>(e->dct.p)}, {SCAL_DOUBLES, (words + 1) / 2}};
}

// `words_cleared`: the launch that prepared the points has cleared the control words already (EvalPlan::prezero)
int eval_tiles(gmb_engine* e, hipStream_t s, bool with_chol, bool words_cleared) {
  const FactorRef f = train_factor(e);
  const int nct = (int)(e->Np / TILE), nrt = (int)(e->Nr / TILE);
  int rc;
  // The ticket counter runs ahead of the factorisation's latency chain by about as many tasks as there are workgroups: an
  // inverse task drawn before its diagonal block L(c, c) exists would sit on a compute unit waiting for it (lag 1 at
  // N = 10k: 75 us median per task, 18.3 ms per evaluation; a quarter of the block columns behind: none, 16.3 ms;
  // tools/gpu_eval_lag.py)
  const int lag = e->et_lag >= 0 ? e->et_lag : std::max(2, std::min(24, nct / 4));
  int nw = 8;
#ifdef GMB_TUNING
  if (const char* cw = getenv("GMB_ET_WAVES")) nw = atoi(cw) == 4 ? 4 : 8;
#endif
  // (a traced launch keeps the list its stamps are decoded with; the pair task exists for eight-wave workgroups only -- ADVICE r05)
  const int pairs = (nw == 8 && !e->ct_trace && (e->et_pairs > 0 || (e->et_pairs < 0 && nct >= e->et_pairs_min_blocks))) ? 1 : 0;
  if (e->et_key[0] != nct || e->et_key[1] != nrt || e->et_key[2] != (int)with_chol || e->et_key[3] != lag || e->et_key[4] != pairs) {
    std::vector<uint32_t> list;
    et_build_tasks(nct, nrt, with_chol, lag, list, pairs != 0);
    if ((rc = e->det_tasks.reserve(e->pool, (int64_t)list.size()))) return rc;
    HIP_TRY(e, hipMemcpy(e->det_tasks, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    e->et_key[0] = nct;
    e->et_key[1] = nrt;
    e->et_key[2] = (int)with_chol;
    e->et_key[3] = lag;
    e->et_key[4] = pairs;
    e->et_ntasks = (int)list.size();
  }
  const int ntasks = e->et_ntasks;
  const int64_t chol_words = (int64_t)nrt * nct + 3 * (int64_t)nct;
  const int64_t words = eval_tiles_words(nct, nrt);
  if ((rc = e->dct.reserve(e->pool, words + 2))) return rc;
  if ((rc = e->dW.reserve(e->pool, e->Np * e->Np))) return rc;
  e->fs.inverse_rewrites_u();  // (Sigma^-1 takes dW; U is marked again once the launch is known to have succeeded)
  if ((rc = e->dUdiag.reserve(e->pool, (int64_t)nct * TILE * TILE))) return rc;
  if ((rc = e->dApart.reserve(e->pool, (int64_t)nct * nct * TILE + nct))) return rc;  // (+ the partials of |v|^2)
  if ((rc = grad_workspace(e))) return rc;
  if (!(with_chol && words_cleared)) HIP_TRY(e, hipMemsetAsync(e->dct, 0, (size_t)words * sizeof(uint32_t), s));
  // a factor that is final already: every tile flag reads "final" (any non-zero word)
  if (!with_chol) HIP_TRY(e, hipMemsetAsync(e->dct + 4, 1, (size_t)nrt * nct * sizeof(uint32_t), s));
  const int lose = with_chol ? e->ct_lose : 0;
  e->chol.injected = lose > 0;
  if (lose > 0) {
    e->ct_lose = 0;
    if ((rc = tiles_lose_tickets(e, s, e->dct, lose))) return rc;
  }
  CholTilesArgs a = tiles_args(f, 0, nct, nrt, ntasks);
  e->chol.traced = e->ct_trace;
  if (e->ct_trace && (rc = tiles_trace_buffer(e, s, a))) return rc;
  EvalTilesArgs x{};
  x.tasks = e->det_tasks;
  x.ntasks = ntasks;
  x.uflags = e->dct + 4 + chol_words;
  x.udiag = e->dUdiag;
  x.Z = e->dW;
  x.ldz = e->Np;
  x.apart = e->dApart;
  x.yb = (int)(e->N / TILE);
  x.rowdone = x.uflags + (int64_t)nct * nct;
  x.alpha = e->dalpha;
  x.v = e->dv;
  x.vpart = e->dApart + (int64_t)nct * nct * TILE;
  x.scal = e->dscal + 1;
  x.with_v = with_chol ? 1 : 0;  // v = L^-1 y with |v|^2, which gmb_factorize takes with extract_v_kernel
  double flops = with_chol ? chol_tiles_flops(f, nct, nrt) : 0.0;
  for (int c = 0; c < nct; ++c)                                                                                       // INV column c
    flops += 2.0 * TILE * TILE * TILE * 0.5 * (double)c * (double)(c + 1) * (c == nct - 1 ? ragged_col_frac(f) : 1.0);
  for (int I = 0; I < nct; ++I) flops += 2.0 * TILE * TILE * TILE * (double)(nct - I) * (double)(I + 1);             // ZZ block row I
  const int grid = (int)std::min<long long>(ntasks, nw == 8 ? e->wg_slots / 2 : e->wg_slots);
  ev_begin(e, s, EV_EVAL_TILES, flops, nct, nrt, (int)e->Np, with_chol ? 1 : 0);
  if (nw == 8) hipLaunchKernelGGL(eval_tiles_kernel<8>, dim3(grid), dim3(512), 0, s, a, x);
#ifdef GMB_TUNING
  else hipLaunchKernelGGL(eval_tiles_kernel<4>, dim3(grid), dim3(256), 0, s, a, x);
#endif
  ev_end(e);
  HIP_TRY(e, hipGetLastError());
  e->chol.tiles = true;
  e->chol.ntasks = ntasks;
  return GMB_OK;
}

// ---- cross-stream ordering helpers -----------------------------------------------------------
hipEvent_t next_sync_event(gmb_engine* e) {
  if (e->sync_next == e->sync_pool.size()) {
    hipEvent_t ev = nullptr;
    (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    e->sync_pool.push_back(ev);
  }
  return e->sync_pool[e->sync_next++];
}
hipEvent_t next_time_event(gmb_engine* e) {  // timing-enabled, reused from call to call
  if (e->time_next == e->time_pool.size()) {
    hipEvent_t ev = nullptr;
    (void)hipEventCreate(&ev);
    e->time_pool.push_back(ev);
  }
  return e->time_pool[e->time_next++];
}
// everything enqueued on `from` so far happens before anything enqueued on `to` from now on
int order_after(gmb_engine* e, hipStream_t from, hipStream_t to) {
  if (from == to) return GMB_OK;
  hipEvent_t ev = next_sync_event(e);
  HIP_TRY(e, hipEventRecord(ev, from));
  HIP_TRY(e, hipStreamWaitEvent(to, ev, 0));
  return GMB_OK;
}

// Look-ahead Cholesky for SMALL matrices (<= masked_max_blocks block columns, N <= 16k): right-looking over
// panels; the latency-bound chain of panel p+1 (leaves, strips, in-panel products) runs on the main stream
// beside U2(p), the bulk of the trailing update, which runs on the process-wide CU-masked stream (it leaves 4
// compute units of every XCD to the chain).  Larger matrices use the plain recursion (chol_cols over the whole
// matrix, one stream): there the chain is a few per cent of the work, and bulk updates that share the chip with
// chain kernels lose more than the overlap wins -- r02: N = 50k 627 ms with look-ahead (bulk updates at 63
// TF/s) vs 607 ms plain (70.8 TF/s); N = 100k 5.02 vs 4.75 s; N = 24k / 32k 1 % apart; N = 16k equal.
int chol_lookahead_masked(gmb_engine* e, const FactorRef& f) {
  const int nct = (int)(f.Np / TILE), nrt = (int)(f.Nr / TILE);
  const int w = e->panel_blocks;
  hipStream_t mainS = e->stream, bulkS = e->aux[2];
  e->sync_next = 0;
  int rc;
  if ((rc = chol_cols(e, mainS, f, 0, std::min(w, nct), nrt, EV_CHOL_PANEL_GEMM))) return rc;  // (panels: their products belong to the chain)
  for (int c0 = 0; c0 < nct; c0 += w) {
    const int c1 = std::min(c0 + w, nct);
    const int n0 = c1, n1 = std::min(c1 + w, nct);
    if (n0 >= nct) break;
    auto update = [&](hipStream_t s, int col_lo, int col_hi) {
      GemmArgs g{};
      g.C = f.A + (int64_t)col_lo * TILE + (int64_t)col_lo * TILE * f.ld;
      g.ldc = f.ld;
      g.A = f.A + (int64_t)col_lo * TILE + (int64_t)c0 * TILE * f.ld;
      g.lda = f.ld;
      g.B = g.A;
      g.ldb = f.ld;
      g.mt = col_hi - col_lo;
      g.nt = nrt - col_lo;
      g.k = (c1 - c0) * TILE;
      g.alpha = -1.0;
      g.beta = 1.0;
      g.tri = 1;
      return launch_gemm(e, s, g, EV_CHOL_UPDATE);
    };
    if ((rc = order_after(e, bulkS, mainS))) return rc;   // U2(p-1) reached these columns
    if ((rc = update(mainS, n0, n1))) return rc;          // U1
    if ((rc = order_after(e, mainS, bulkS))) return rc;
    if (n1 < nct && (rc = update(bulkS, n1, nct))) return rc;  // U2, on the compute units its mask allows
    if ((rc = chol_cols(e, mainS, f, n0, n1, nrt, EV_CHOL_PANEL_GEMM))) return rc;  // panel p+1, beside U2
  }
  return order_after(e, bulkS, mainS);
}

// what the caller of a factorisation asks for beyond the matrix
struct CholOpts {
  bool masked_ok = false;  // the masked look-ahead may be chosen (the training factorisation only: C has never been factored on it)
  bool trace = false;      // a whole-matrix tile launch stamps its tasks (gmb_chol_task_trace)
  int lose = 0;            // ... and loses its first tickets (gmb_debug_chol_lose_tickets); `res->injected` says it took them
};

// f -> L in place on e->stream, by the schedule its size asks for: the persistent tile kernel from tiles_min_blocks to
// tiles_max_blocks block columns (or under scheme 3), the masked look-ahead where allowed, else the plain recursion with its
// bottom panels as launches of the tile kernel.  Nothing is synchronised; `res` (cleared by the caller) says what to read back.
int chol_factor(gmb_engine* e, const FactorRef& f, const CholOpts& o, CholResult* res) {
  const int nblocks = (int)(f.Np / TILE), nrt = (int)(f.Nr / TILE);
  const bool tiles = !e->naive_leaf && (e->chol_scheme == 3 || (e->chol_scheme < 0 && nblocks >= e->tiles_min_blocks &&
                                                                 nblocks <= e->tiles_max_blocks));
  const bool masked = o.masked_ok && !tiles && e->lookahead && e->aux_shared && nblocks > e->panel_blocks &&
                      (e->chol_scheme == 2 || (e->chol_scheme < 0 && nblocks <= e->masked_max_blocks));
  if (tiles) return chol_tiles(e, e->stream, f, o.trace, o.lose, res);
  if (masked) return chol_lookahead_masked(e, f);
  const bool tile_panels = !e->naive_leaf && !e->panel_tiles_veto && e->panel_tiles_w >= 2 && e->chol_scheme != 0;
  if (tile_panels) {
    int rc;
    if ((rc = f.ct->reserve(e->pool, 4 + (int64_t)(e->panel_tiles_w + 3) * nrt))) return rc;
    HIP_TRY(e, hipMemsetAsync(*f.ct, 0, 4 * sizeof(uint32_t), e->stream));  // (the abort word: once per factorisation)
  }
  return chol_cols(e, e->stream, f, 0, nblocks, nrt, EV_CHOL_UPDATE, tile_panels ? res : nullptr);
}

// ---- predict recursion: V <- W L^-T over column blocks [c0, c1) ------------------------------
// lfirst / lstride (optional): row tile t of V stands for block row lfirst + t*lstride of a matrix
// whose rows are zero left of their own diagonal block (rows of the identity being solved into
// rows of L^-T): the update products then skip the structurally zero part of their contraction.
int trsm_cols(gmb_engine* e, hipStream_t s, const FactorRef& f, double* V, int64_t ldz, int ntm, int c0, int c1, EvKind kind_gemm, EvKind kind_strip,
              int lfirst = -1, int lstride = 0) {
  if (c1 - c0 == 1)
    return launch_trsm_strip(e, s, V + (int64_t)c0 * TILE * ldz, ldz, (int64_t)ntm * TILE,
                             f.A + (int64_t)c0 * TILE * (f.ld + 1), f.ld, f.dinv16 + (int64_t)c0 * 8 * 256,
                             (int)std::min<int64_t>(TILE, f.N - (int64_t)c0 * TILE), kind_strip);
  const int mid = c0 + (c1 - c0 + 1) / 2;
  int rc = trsm_cols(e, s, f, V, ldz, ntm, c0, mid, kind_gemm, kind_strip, lfirst, lstride);
  if (rc) return rc;
  GemmArgs g{};
  g.C = V + (int64_t)mid * TILE * ldz;
  g.ldc = ldz;
  g.A = f.A + (int64_t)mid * TILE + (int64_t)c0 * TILE * f.ld;
  g.lda = f.ld;
  g.B = V + (int64_t)c0 * TILE * ldz;
  g.ldb = ldz;
  g.mt = c1 - mid;
  g.nt = ntm;
  g.k = (mid - c0) * TILE;
  g.alpha = -1.0;
  g.beta = 1.0;
  if (lstride > 0) {
    g.klo_n = 1;
    g.krow_stride = lstride;
    g.krow_off = (lfirst - c0) * TILE;
  }
  rc = launch_gemm(e, s, g, kind_gemm);
  if (rc) return rc;
  return trsm_cols(e, s, f, V, ldz, ntm, mid, c1, kind_gemm, kind_strip, lfirst, lstride);
}

// ---- NLML gradient ---------------------------------------------------------------------------
// Triangular inverse by recursive block inversion, kept in BOTH orientations so that every
// product is a k-major ("NT") MFMA GEMM with fully coalesced operand loads:
//   W = L^-1   (lower) in e->dW,
//   U = L^-T   (upper) in the upper triangle + diagonal tiles of the factor buffer e->dA
//              (the diagonal blocks of L are no longer needed once inv(L_kk) exists; the
//              off-diagonal blocks of L stay intact in the lower triangle).
//   [[A,0],[B,C]]^-1 = [[A^-1,0],[-C^-1 B A^-1, C^-1]]:
//     T^T = U_A B^T (scratch, mirrored region of dW),  W21 = -W_C T,  U12 = W21^T (transpose).
int launch_transpose(gmb_engine* e, hipStream_t s, const double* src, int64_t lds_, double* dst, int64_t ldd, int rows,
                     int cols) {
  hipLaunchKernelGGL(transpose_kernel, dim3((rows + 31) / 32, (cols + 31) / 32), dim3(256), 0, s, src,
                     lds_, dst, ldd, rows, cols);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

int winv_node(gmb_engine* e, hipStream_t s, int c0, int c1, bool recurse);

int winv_cols(gmb_engine* e, hipStream_t s, int c0, int c1) { return winv_node(e, s, c0, c1, true); }

// The two halves of a node are independent (both read only L and the inv(L_kk) blocks), so the
// whole recursion tree can be executed level by level, bottom-up, with the nodes of a level dealt
// round-robin over four streams: the many small GEMMs at the bottom of the tree (a few tiles
// each) run side by side instead of one after the other.
struct InvNode {
  int c0, c1;
};
void collect_inv_nodes(int c0, int c1, int depth, std::vector<std::vector<InvNode>>& levels) {
  if ((int)levels.size() <= depth) levels.resize(depth + 1);
  levels[depth].push_back(InvNode{c0, c1});
  if (c1 - c0 > 1) {
    const int mid = c0 + (c1 - c0 + 1) / 2;
    collect_inv_nodes(c0, mid, depth + 1, levels);
    collect_inv_nodes(mid, c1, depth + 1, levels);
  }
}
int build_inv_plan(gmb_engine* e, const std::vector<std::vector<InvNode>>& levels);
int winv_level_batched(gmb_engine* e, hipStream_t s, const gmb_engine::InvLevelPlan& lp);

int winv_levels(gmb_engine* e, int nt) {
  std::vector<std::vector<InvNode>> levels;
  collect_inv_nodes(0, nt, 0, levels);
  hipStream_t streams[4] = {e->stream, e->aux[0], e->aux[1], e->aux_shared ? e->aux[0] : e->aux[2]};
  // Small matrices (<= 64 block columns): only the two top levels are not batched, i.e. at most two nodes could run
  // side by side -- less than the event records / stream waits of the fork and the joins cost on the host, which is
  // what such a gradient is bound by (timeline at N = 2048: 70 us of idle GPU before the first batched level).  One
  // stream, no events.
  if (nt <= 64) streams[1] = streams[2] = streams[3] = e->stream;
  int rc;
  for (int a = 1; a < 4; ++a)
    if ((rc = order_after(e, streams[0], streams[a]))) return rc;
  const bool batched = e->batch_inverse && build_inv_plan(e, levels) == GMB_OK;
  bool aux_behind = false;  // the main stream has run batched levels the auxiliary streams have not waited for
  for (int depth = (int)levels.size() - 1; depth >= 0; --depth) {
    if (batched && e->inv_plan[depth].count > 0) {
      // consecutive batched levels live on the main stream alone: no event traffic between them (an
      // event record + three stream waits per level showed up as 20-25 us bubbles in the timeline)
      // (every stream was joined into the main one after the previous level)
      if ((rc = winv_level_batched(e, streams[0], e->inv_plan[depth]))) return rc;
      aux_behind = true;
      continue;
    }
    if (aux_behind) {
      for (int a = 1; a < 4; ++a)
        if ((rc = order_after(e, streams[0], streams[a]))) return rc;
      aux_behind = false;
    }
    int idx = 0;
    for (const InvNode& nd : levels[depth])
      if ((rc = winv_node(e, streams[levels[depth].size() > 1 ? (idx++ & 3) : 0], nd.c0, nd.c1, false))) return rc;
    for (int a = 1; a < 4; ++a)
      if ((rc = order_after(e, streams[a], streams[0]))) return rc;
    if (depth > 0)
      for (int a = 1; a < 4; ++a)
        if ((rc = order_after(e, streams[0], streams[a]))) return rc;
  }
  return GMB_OK;
}

// The two products and the transpose of one merge node [c0, c1) of the inverse tree.
void winv_node_products(gmb_engine* e, int c0, int c1, GemmArgs& gt, GemmArgs& gw, TransposeJob& tr) {
  const int64_t ldw = e->Np, lda = e->ld;
  double* W = e->dW;
  double* A = e->dA;
  const int mid = c0 + (c1 - c0 + 1) / 2;
  const int n1 = mid - c0, n2 = c1 - mid;
  // T^T[j][r] = sum_{k>=j} U_A[j][k] * B[r][k]   -> scratch at W[c0.., mid..]
  gt = GemmArgs{};
  gt.C = W + (int64_t)c0 * TILE + (int64_t)mid * TILE * ldw;
  gt.ldc = ldw;
  gt.A = A + (int64_t)mid * TILE + (int64_t)c0 * TILE * lda;  // B = L21
  gt.lda = lda;
  gt.B = A + (int64_t)c0 * TILE + (int64_t)c0 * TILE * lda;   // U_A (upper triangle of the factor buffer)
  gt.ldb = lda;
  gt.mt = n2;
  gt.nt = n1;
  gt.k = n1 * TILE;
  gt.klo_n = 1;
  gt.alpha = 1.0;
  gt.beta = 0.0;
  gt.nblk_stride = 1;
  // W21[r][j] = -sum_{s<=r} W_C[r][s] * T^T[j][s]
  gw = GemmArgs{};
  gw.C = W + (int64_t)mid * TILE + (int64_t)c0 * TILE * ldw;
  gw.ldc = ldw;
  gw.A = W + (int64_t)c0 * TILE + (int64_t)mid * TILE * ldw;   // T^T
  gw.lda = ldw;
  gw.B = W + (int64_t)mid * TILE + (int64_t)mid * TILE * ldw;  // W_C
  gw.ldb = ldw;
  gw.mt = n1;
  gw.nt = n2;
  gw.k = n2 * TILE;
  gw.khi_n = 1;
  gw.alpha = -1.0;
  gw.beta = 0.0;
  gw.nblk_stride = 1;
  // U12 = W21^T into the upper triangle of the factor buffer
  tr.src = W + (int64_t)mid * TILE + (int64_t)c0 * TILE * ldw;
  tr.dst = A + (int64_t)c0 * TILE + (int64_t)mid * TILE * lda;
  tr.rows = n2 * TILE;
  tr.cols = n1 * TILE;
}

int winv_node(gmb_engine* e, hipStream_t s, int c0, int c1, bool recurse) {
  if (c1 - c0 == 1) return GMB_OK;  // leaf_invert_kernel wrote both diagonal blocks already
  const int mid = c0 + (c1 - c0 + 1) / 2;
  int rc;
  if (recurse) {
    if ((rc = winv_node(e, s, c0, mid, true))) return rc;
    if ((rc = winv_node(e, s, mid, c1, true))) return rc;
  }
  GemmArgs gt, gw;
  TransposeJob tr;
  winv_node_products(e, c0, c1, gt, gw, tr);
  if ((rc = launch_gemm(e, s, gt, EV_GRAD_GEMM))) return rc;
  if ((rc = launch_gemm(e, s, gw, EV_GRAD_GEMM))) return rc;
  return launch_transpose(e, s, tr.src, e->Np, tr.dst, e->ld, tr.rows, tr.cols);
}

// ---- batched levels ---------------------------------------------------------------------------
// Levels of the tree with at least MIN_BATCH_NODES merge nodes run as three launches (all T^T
// products, all W21 products, all transposes) whose descriptors are built once per data set.
constexpr int MIN_BATCH_NODES = 4;

int build_inv_plan(gmb_engine* e, const std::vector<std::vector<InvNode>>& levels) {
  if (e->plan_N == e->N && e->plan_ld == e->ld && e->plan_Np == e->Np && e->plan_W == e->dW && e->plan_A == e->dA)
    return GMB_OK;
  std::vector<GemmArgs> hg;
  std::vector<TransposeJob> ht;
  e->inv_plan.assign(levels.size(), gmb_engine::InvLevelPlan{});
  static const int BMs[3] = {128, 64, 128}, BNs[3] = {128, 64, 64};
  static const double rate[3] = {73.0, 63.0, 65.0};
  static const int per128[3] = {1, 4, 2};
  for (size_t depth = 0; depth < levels.size(); ++depth) {
    std::vector<InvNode> nodes;
    for (const InvNode& nd : levels[depth])
      if (nd.c1 - nd.c0 > 1) nodes.push_back(nd);
    if ((int)nodes.size() < MIN_BATCH_NODES) continue;
    gmb_engine::InvLevelPlan& lp = e->inv_plan[depth];
    lp.count = (int)nodes.size();
    std::vector<GemmArgs> gs[2];
    lp.toff = (int64_t)ht.size();
    for (const InvNode& nd : nodes) {
      GemmArgs gt, gw;
      TransposeJob tr;
      winv_node_products(e, nd.c0, nd.c1, gt, gw, tr);
      gs[0].push_back(gt);
      gs[1].push_back(gw);
      ht.push_back(tr);
      lp.tr_rows = std::max(lp.tr_rows, tr.rows);
      lp.tr_cols = std::max(lp.tr_cols, tr.cols);
    }
    for (int b = 0; b < 2; ++b) {
      long long nact = 0;
      for (const GemmArgs& g : gs[b]) nact += gemm_nact128(g);
      int variant = 0;
      double best = 0.0;
      for (int v = 0; v < 3; ++v) {  // the launch_gemm model on the level's total tile count
        const double t = (double)(nact * per128[v]);
        const double sc = rate[v] * per128[v] / std::max(1.0, t / (double)e->wg_slots + 0.5);
        if (sc > best) {
          best = sc;
          variant = v;
        }
      }
      lp.variant[b] = variant;
      lp.off[b] = (int64_t)hg.size();
      for (GemmArgs g : gs[b]) {
        g.mt = g.mt * TILE / BMs[variant];
        g.nt = g.nt * TILE / BNs[variant];
        g.order = e->lpt_order ? (b == 0 ? 1 : 2) : 0;
        double fl = 0.0;
        const int nb = gemm_schedule(g, BMs[variant], BNs[variant], &fl);
            lp.grid_x[b] = std::max(lp.grid_x[b], nb);
        lp.flops[b] += fl;
        hg.push_back(g);
      }
    }
  }
  e->dplan_gemm.drop(e->pool);
  e->dplan_tr.drop(e->pool);
  e->plan_N = -1;
  if (!hg.empty()) {
    int rc;
    if ((rc = e->dplan_gemm.renew(e->pool, (int64_t)hg.size(), false)) || (rc = e->dplan_tr.renew(e->pool, (int64_t)ht.size(), false))) return rc;
    HIP_TRY(e, hipMemcpy(e->dplan_gemm, hg.data(), hg.size() * sizeof(GemmArgs), hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(e->dplan_tr, ht.data(), ht.size() * sizeof(TransposeJob), hipMemcpyHostToDevice));
  }
  e->plan_N = e->N;
  e->plan_ld = e->ld;
  e->plan_Np = e->Np;
  e->plan_W = e->dW;
  e->plan_A = e->dA;
  return GMB_OK;
}

int winv_level_batched(gmb_engine* e, hipStream_t s, const gmb_engine::InvLevelPlan& lp) {
  for (int b = 0; b < 2; ++b) {
    if (lp.grid_x[b] <= 0) continue;
    const GemmArgs* batch = e->dplan_gemm + lp.off[b];
    const dim3 grid(lp.grid_x[b], lp.count);
    ev_begin(e, s, EV_GRAD_GEMM, lp.flops[b], lp.count, 0, 0, (lp.variant[b] << 8) | 64);
    switch (lp.variant[b]) {
      case 0: hipLaunchKernelGGL((gemm_f64_batched_kernel<2, 2, 4, 4, 2>), grid, dim3(256), 0, s, batch); break;
      case 1: hipLaunchKernelGGL((gemm_f64_batched_kernel<2, 2, 2, 2, 2>), grid, dim3(256), 0, s, batch); break;
      default: hipLaunchKernelGGL((gemm_f64_batched_kernel<2, 2, 4, 2, 2>), grid, dim3(256), 0, s, batch); break;
    }
    ev_end(e);
    HIP_TRY(e, hipGetLastError());
  }
  hipLaunchKernelGGL(transpose_batched_kernel, dim3((lp.tr_rows + 31) / 32, (lp.tr_cols + 31) / 32, lp.count),
                     dim3(256), 0, s, e->dplan_tr + lp.toff, e->Np, e->ld);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// one term's trace reductions: the direct-loop tiles, and behind them the interior tiles of a split pass (kinds 0 - 2 only)
int launch_grad(gmb_engine* e, const GradArgs& a_in, int nblocks) {
  const dim3 grid(nblocks), block(256);
  const size_t lds = grad_lds_bytes(e->nc_pad, a_in.p.n_lin, a_in.p.n_tab);
  GradArgs a = a_in;
  a.part_block0 = 0;
  const int gs = a.gsplit > 1 ? a.gsplit : 1;
  const dim3 grid0((a.split ? a.general_tiles : nblocks) * gs);  // (split: one tile of the general-tile list per gs workgroups)
  // (two launches, so the kind and the width are taken apart: the kind once, the width for each launch)
  const bool known = with_kind(a.p.kind, [&](auto kind) {
    constexpr int K = decltype(kind)::value;
    with_nc(e->nc_pad, [&](auto nc) { hipLaunchKernelGGL((grad_tile_kernel<K, decltype(nc)::value>), grid0, block, lds, e->stream, a); });
    if constexpr (K <= 2) {
      if (a.split) {  // the interior tiles on the matrix pipe: runs of the full enumeration, the partial vectors behind the first set
        a.part_block0 = a.general_tiles * gs;
        with_nc(e->nc_pad, [&](auto nc) { hipLaunchKernelGGL((grad_interior_kernel<K, decltype(nc)::value>), grid, block, 0, e->stream, a); });
      }
    }
  });
  if (!known) return fail(e, GMB_EINVAL, "unknown kernel kind %d", a.p.kind);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// ---- gradient building blocks ---------------------------------------------------------------------
// (a) grad_sigma_inv_rows: block rows shard, shard + nshards, ... of Sigma^-1 = U U^T (lower triangle) from
//     U = L^-T in the upper triangle of the factor buffer, into Z -- the full Np x Np matrix (packed = false:
//     rows at their global position, ldz = Np) or ONLY the owned rows, packed (multi-GPU: ldz = owned * 128);
// (b) grad_reduce: the fused trace reductions over those rows, one pass per covariance term (additive models
//     have several); term t accumulates into region t of dgpart: [ls.. | eta | tau | c.. ] at 0, its tables
//     from 64.  `h` receives the raw accumulators: plain sums over tiles, so shards of several GPUs add up.
int grad_workspace(gmb_engine* e) {
  int rc;
  if ((rc = e->dalpha.reserve(e->pool, 3 * e->Np))) return rc;  // alpha | the refinement's residual t | its correction (refine_alpha)
  return GMB_OK;  // (the accumulators live in the engine's scalar block)
}

int grad_sigma_inv_rows(gmb_engine* e, hipStream_t s, int shard, int nshards, double* Z, int64_t ldz, bool packed) {
  const int nt = (int)(e->Np / TILE);
  const int owned = shard < nt ? (nt - shard + nshards - 1) / nshards : 0;
  GemmArgs g{};
  g.C = packed ? Z : Z + (int64_t)shard * TILE;
  g.ldc = ldz;
  g.A = e->dA;
  g.lda = e->ld;
  g.B = e->dA + (int64_t)shard * TILE;
  g.ldb = e->ld;
  g.mt = nt;
  g.nt = owned;
  g.k = (int)e->Np;
  g.klo_n = 1;
  g.krow_off = shard * TILE;
  g.tri = 1;
  g.tri_off = shard * TILE;
  g.nblk_stride = nshards;
  g.cblk_stride = packed ? 1 : 0;
  g.alpha = 1.0;
  g.beta = 0.0;
  return launch_gemm(e, s, g, EV_GRAD_GEMM);
}

// how a pass of grad_reduce begins and ends.  Default (gmb_nlml, the multi-GPU drivers): it clears its accumulators and copies them to `h`.
struct GradLanding {
  bool acc_cleared = false;  // the accumulators are clear already: the evaluation's one memset, or its preparation launch
  bool by_kernel = false;    // the results land in the pinned block (eval_land_kernel / grad_finish_kernel): gmb_evaluate's light path
};

int grad_reduce(gmb_engine* e, int shard, int nshards, const double* Z, int64_t ldz, bool packed,
                std::vector<double>& h, const GradLanding& landing) {
  const gmb_kernel_spec& s = e->spec;
  const int nt = (int)(e->Np / TILE);
  if (!landing.acc_cleared) HIP_TRY(e, hipMemsetAsync(e->dgpart, 0, (GACC_DOUBLES + 64) * sizeof(double), e->stream));
  const int n_ls = s.ard ? s.n_cont : 1;
  long long total = 0;
  for (int i = shard; i < nt; i += nshards) total += i + 1;
  // persistent workgroups: six per compute unit, each reduces a contiguous run of `per` tiles in registers / LDS
  // and writes ONE partial vector; a second launch adds the vectors in a fixed order (bit-reproducible results)
  const long long want = std::max<long long>(1, 3 * e->wg_slots);  // 6 workgroups per compute unit: one resident round
  const int per = (int)std::max<long long>(1, (total + want - 1) / want);
  const int grid = (int)((total + per - 1) / per);
  const int ncp = e->nc_pad;
  bool merged = false;  // the pass ends in grad_finish_kernel (set inside the one term's iteration)
  GradFinishArgs fin{};
  const int walked = walk_terms(e, [&](int t) -> int {
    const gmb_engine::Term& tr = e->terms[t];
    int rc;
    GradArgs a{};
    a.p = tr.cp;
    a.pts = train_set(e);
    a.Z = Z;
    a.ldz = ldz;
    a.z_packed = packed ? 1 : 0;
    a.alpha = e->dalpha;
    a.tiles = nt;
    a.ard = s.ard;
    // d r^2 / d ls = -2 r^2 / ls per prepared column whatever constant the preparation's weight carries: the gradient's factor
    // is the TRUE 1 / ls_d -- the weight itself, or twice it for pm.gp.cov.Periodic (apply_theta)
    const int ncols = e->periodic ? 2 * s.n_cont : s.n_cont;  // prepared columns
    const double true_inv = e->periodic == 2 ? 2.0 : 1.0;
    a.nc_real = ncols;
    for (int k = 0; k < 16; ++k) a.inv_ls[k] = k < ncols ? true_inv * tr.pa.inv_ls[k] : 0.0;
    a.eta = tr.eta;
    a.row_first = shard;
    a.row_stride = nshards;
    a.total_tiles = total;
    a.per = per;
    const int n_small = ncp + 2 + tr.cp.n_lin;
    a.part_stride = n_small + tr.cp.n_tab * 64;
    double* acc = e->dgpart + (int64_t)t * GACC_REGION;
    int tab_acc_off[MAX_TABS] = {0};
    int off = 64, big = 0;
    for (int j = 0; j < tr.cp.n_tab; ++j) {
      tab_acc_off[j] = off;
      const int LL = tr.cp.tab_levels[j] * tr.cp.tab_levels[j];
      off += LL;
      a.big_off[j] = big;
      if (tr.cp.tab_levels[j] > 8) big += LL;
    }
    a.big_stride = big;
    // smooth stationary terms: the full tiles strictly below the diagonal go to grad_interior_kernel (gradient.hpp)
    a.split = (tr.cp.kind == GMB_EXPQUAD || tr.cp.kind == GMB_MATERN52 || tr.cp.kind == GMB_MATERN32) && tr.cp.n_lin == 0 &&
                      tr.cp.n_tab == 0 && !e->naive_leaf
                  ? 1 : 0;
    // the tiles the interior launch leaves: the diagonal tile of every owned block row + a ragged last row's other tiles
    a.n_owned_rows = shard < nt ? (nt - shard + nshards - 1) / nshards : 0;
    const bool last_ragged_owned = e->Np > e->N && (nt - 1 - shard) % nshards == 0 && nt - 1 >= shard;
    a.general_tiles = a.n_owned_rows + (last_ragged_owned ? nt - 1 : 0);
    if (a.general_tiles == 0) a.split = 0;
    // small matrices: every tile through the direct loops of ONE launch, four workgroups per tile (N = 392: the interior launch's
    // 10.8 us behind the general tiles' 10.3 saved; from 129 tiles on the matrix-pipe form wins)
    if (total <= 128) a.split = 0;
    // small launches: four workgroups per direct-loop tile (GradArgs::gsplit)
    const int ndirect = a.split ? a.general_tiles : grid;  // runs / list tiles of grad_tile_kernel
    a.gsplit = ndirect <= 512 ? 4 : 1;
    const int nvec = a.split ? ndirect * a.gsplit + grid : ndirect * a.gsplit;  // partial vectors the pass leaves
    if (grid > 0) {
      if ((rc = e->dgred.reserve(e->pool, (int64_t)nvec * a.part_stride))) return rc;
      a.part = e->dgred;
      if (big > 0) {
        if ((rc = e->dgbig.reserve(e->pool, (int64_t)ndirect * a.gsplit * 4 * big))) return rc;
        HIP_TRY(e, hipMemsetAsync(e->dgbig, 0, (size_t)ndirect * a.gsplit * 4 * big * sizeof(double), e->stream));
        a.big = e->dgbig;
      }
      if ((rc = launch_grad(e, a, grid))) return rc;
      // second stage: dense slots of the partial vectors -> the term's accumulator region
      GradRanges r{};
      auto add = [&](int dense, int count, int dst) {
        r.dense[r.n] = dense;
        r.count[r.n] = count;
        r.dst[r.n] = dst;
        ++r.n;
      };
      double* tmp = e->dgpart + GACC_DOUBLES;  // scratch behind the accumulators
      merged = landing.by_kernel && e->terms.size() == 1 && s.ard && !e->periodic && big == 0 && nvec <= 8192 && e->N <= 16384;
      if (e->periodic) add(0, ncols, (int)(tmp - acc));      // per-column sums, folded into the dimensions' parameters below
      else if (s.ard) add(0, s.n_cont, 0);
      else add(0, s.n_cont, (int)(tmp - acc));               // per-dimension sums, folded into the one parameter below
      add(ncp, 2 + tr.cp.n_lin, n_ls);                        // eta | tau | c..
      for (int j = 0; j < tr.cp.n_tab; ++j)
        if (tr.cp.tab_levels[j] <= 8) add(n_small + j * 64, tr.cp.tab_levels[j] * tr.cp.tab_levels[j], tab_acc_off[j]);
      if (merged) {
        // small evaluation: the second stage, the diagonal terms and the landing are ONE launch (grad_finish_kernel)
        fin.part = e->dgred;
        fin.nparts = nvec;
        fin.nslots = a.part_stride;
        fin.stride = a.part_stride;
        fin.r = r;
        fin.acc = acc;
      } else {
        hipLaunchKernelGGL(grad_sum_partials_kernel, dim3(a.part_stride), dim3(256), 0, e->stream, e->dgred, nvec,
                           (int64_t)a.part_stride, r, acc);
      }
      if (e->periodic) hipLaunchKernelGGL(grad_fold_periodic_kernel, dim3(1), dim3(64), 0, e->stream, acc, s.n_cont, (int)s.ard, tmp);
      else if (!s.ard) hipLaunchKernelGGL(grad_fold_ls_kernel, dim3(1), dim3(64), 0, e->stream, acc, s.n_cont, tmp);
      if (big > 0) {
        GradRanges rb{};
        for (int j = 0; j < tr.cp.n_tab; ++j)
          if (tr.cp.tab_levels[j] > 8) {
            rb.dense[rb.n] = a.big_off[j];
            rb.count[rb.n] = tr.cp.tab_levels[j] * tr.cp.tab_levels[j];
            rb.dst[rb.n] = tab_acc_off[j];
            ++rb.n;
          }
        hipLaunchKernelGGL(grad_sum_partials_kernel, dim3(big), dim3(256), 0, e->stream, e->dgbig, ndirect * a.gsplit * 4, (int64_t)big, rb, acc);
      }
      HIP_TRY(e, hipGetLastError());
    }
    if (t == 0) {  // diagonal terms (sigma, noise table) with the global term's categories in place
      const double sigma = e->theta[n_ls + 1];
      if (merged) {
        fin.Z = Z;
        fin.ldz = ldz;
        fin.alpha = e->dalpha;
        fin.pts = train_set(e);
        fin.p = tr.cp;
        fin.sigma = sigma;
        fin.diag_out = e->dgpart + off;
      } else {
        hipLaunchKernelGGL(grad_diag_kernel, dim3(1), dim3(1024), 0, e->stream, Z, ldz, e->dalpha, train_set(e),
                           tr.cp, sigma, e->dgpart + off, shard, nshards, packed ? 1 : 0);
        HIP_TRY(e, hipGetLastError());
      }
    }
    return GMB_OK;
  });
  if (walked) return walked;
  h.assign(GACC_DOUBLES, 0.0);
  if (landing.by_kernel) {
    // gmb_evaluate on the fused launch: scalars, failure index, abort word and the used head of every accumulator region go to
    // the pinned landing in one launch; grad_accumulate hands them on after its synchronisation
    EvalLandArgs la{};
    la.scal = e->dscal;
    la.info = e->dinfo;
    la.abort = e->chol.tiles ? e->dct + 1 : nullptr;
    la.gacc = e->dgpart;
    la.nterms = (int)e->terms.size();
    la.region = GACC_REGION;
    for (size_t t = 0; t < e->terms.size(); ++t) {
      int used = 64;
      for (int j = 0; j < e->terms[t].cp.n_tab; ++j) used += e->terms[t].cp.tab_levels[j] * e->terms[t].cp.tab_levels[j];
      la.used[t] = std::min(used + 64, GACC_REGION);  // (+ the diagonal terms' slots behind the tables)
    }
    la.out_scal = e->hl_dev->scal;
    la.out_info = &e->hl_dev->info;
    la.out_abort = &e->hl_dev->abort;
    la.out_gacc = e->hl_dev->gacc;
    if (merged) {
      fin.land = la;
      hipLaunchKernelGGL(grad_finish_kernel, dim3(1), dim3(1024), 0, e->stream, fin);
    } else hipLaunchKernelGGL(eval_land_kernel, dim3(1), dim3(256), 0, e->stream, la);
    HIP_TRY(e, hipGetLastError());
    return GMB_OK;
  }
  HIP_TRY(e, hipMemcpyAsync(h.data(), e->dgpart, GACC_DOUBLES * sizeof(double), hipMemcpyDeviceToHost,
                            e->stream));
  return GMB_OK;
}

// One refinement step of alpha = L^-T v (gradient.hpp: lt_residual_kernel): t = v - L^T alpha, then alpha += U t with U = L^-T
// by rows in the factor buffer's upper triangle (the tile path: ut_tile_kernel, partial vectors in dApart) or, when W = L^-1
// is given (the recursion: W in dW, lower), alpha += W^T t.
int refine_alpha(gmb_engine* e, const TriOperand& L, const TriOperand* U, const double* W, int64_t ldw) {
  const int nt = (int)(e->Np / TILE);
  double* t = e->dalpha + e->Np;
  hipLaunchKernelGGL(lt_residual_kernel, dim3((unsigned)((e->N + 3) / 4)), dim3(256), 0, e->stream, L, e->dv, e->dalpha, e->N, t);
  if (U) {
    hipLaunchKernelGGL(ut_tile_kernel, dim3(nt, nt), dim3(256), 0, e->stream, *U, t, e->N, e->dApart, e->Np);
    hipLaunchKernelGGL(alpha_add_kernel, dim3((unsigned)((e->N + 255) / 256)), dim3(256), 0, e->stream, e->dalpha, e->dApart,
                       e->Np, nt, 1, e->N);
  } else {
    double* corr = e->dalpha + 2 * e->Np;
    hipLaunchKernelGGL(wt_v_kernel, dim3((unsigned)((e->N + 3) / 4)), dim3(256), 0, e->stream, W, ldw, t, e->N, corr);
    hipLaunchKernelGGL(alpha_add_kernel, dim3((unsigned)((e->N + 255) / 256)), dim3(256), 0, e->stream, e->dalpha, corr,
                       e->Np, 1, 0, e->N);
  }
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// matrices whose inverse / Sigma^-1 run as tile tasks (eval_tiles.hpp): the sizes the tile Cholesky factors
bool grad_by_tiles(const gmb_engine* e) {
  const int nt = (int)(e->Np / TILE);
  if (e->naive_leaf || e->grad_scheme == 0) return false;
  if (e->grad_scheme > 0) return nt >= 1 && nt <= 0x7fff;
  return nt >= e->tiles_min_blocks && nt <= e->tiles_max_blocks;
}

// The launch tree's two halves around whatever reads W = L^-1 in between, on the matrix factored in the factor buffer (the
// training factor; B's of the Laplace path).  tri_inverse_pair: W = L^-1 into dW (lower) and U = L^-T into the factor buffer (upper
// triangle + the diagonal blocks, whose L waits in dDiagSave).  `waits_pending`: the factorisation's cross-stream waits may still be
// pending on pooled events (gmb_evaluate enqueues the gradient behind a factorisation the host has not looked at).
int tri_inverse_pair(gmb_engine* e, bool waits_pending) {
  const int nt = (int)(e->Np / TILE);
  int rc;
  if ((rc = e->dDiagSave.reserve(e->pool, (int64_t)nt * TILE * TILE))) return rc;
  // the diagonal blocks of L are put back at the end: U takes their place in between
  hipLaunchKernelGGL(diag_blocks_copy_kernel, dim3(nt), dim3(256), 0, e->stream, e->dA, e->ld, e->dDiagSave, 1);
  // inverses of all diagonal factor blocks, one workgroup each (kept off the Cholesky's chain)
  {
    InvArgs ia;
    ia.L = e->dA;
    ia.lda = e->ld;
    ia.blk_stride = (int64_t)TILE * (e->ld + 1);
    ia.dinv16 = e->dDinv16;
    ia.invL = nullptr;
    ia.n = e->N;
    ia.W = e->dW;
    ia.ldw = e->Np;
    ia.U = e->dA;
    ia.ldu = e->ld;
    hipLaunchKernelGGL(leaf_invert_kernel, dim3(nt), dim3(256), 0, e->stream, ia);
    HIP_TRY(e, hipGetLastError());
  }
  if (!waits_pending) e->sync_next = 0;
  return e->par_inverse ? winv_levels(e, nt) : winv_cols(e, e->stream, 0, nt);
}

// ... and inverse_from_pair: (L L^T)^-1 = U U^T (lower triangle) into dW -- the last reader of U: the factor's diagonal blocks go back
int inverse_from_pair(gmb_engine* e) {
  const int nt = (int)(e->Np / TILE);
  int rc;
  if (e->Np > e->N)
    hipLaunchKernelGGL(reset_pad_cols_kernel, dim3((unsigned)((e->Np + 255) / 256)), dim3(256), 0, e->stream,
                       e->dA, e->ld, e->N, e->Np);
  HIP_TRY(e, hipGetLastError());
  if ((rc = grad_sigma_inv_rows(e, e->stream, 0, 1, e->dW, e->Np, false))) return rc;
  hipLaunchKernelGGL(diag_blocks_copy_kernel, dim3(nt), dim3(256), 0, e->stream, e->dA, e->ld, e->dDiagSave, 0);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// Single-GPU gradient: W = L^-1 and U = L^-T by recursive block inversion, alpha = W^T v, Sigma^-1 = U U^T
// into dW, reductions.  The factor is consumed.  `job`: the factorisation this gradient is enqueued behind before the host has
// looked at it (gmb_evaluate), or null behind a factor that is final (gmb_nlml, gmb_evaluate's retry).
int grad_accumulate(gmb_engine* e, std::vector<double>& h, FactorJob* job) {
  HIP_TRY(e, hipSetDevice(e->device));
  if (e->fs.consumed())
    return fail(e, GMB_EINVAL, "the factor was already consumed by a gradient call; refactorize");
  int rc;
  gmb_timings& tm = e->tm;
  tm.grad_ms = tm.grad_gemm_ms = tm.grad_gemm_flops = 0.0;
  if ((rc = e->dW.reserve(e->pool, e->Np * e->Np))) return rc;
  if ((rc = grad_workspace(e))) return rc;
  const int nt = (int)(e->Np / TILE);
  const bool fused = job && job->fused_pending;
  if (fused || grad_by_tiles(e)) {
    // Sigma^-1 and the alpha parts come from the persistent evaluation launch: already enqueued with the factorisation
    // (gmb_evaluate), or launched here behind a factor that is final.  L stays intact: nothing to save or restore.
    const bool light = fused;  // (only gmb_evaluate's light plan enqueues it: results land through eval_land_kernel, see grad_reduce)
    const bool timed = !(light && !job->events_recorded);
    std::unique_ptr<PhaseTimer> tgt(timed ? new PhaseTimer(e) : nullptr);
    bool own_launch = false;
    if (!fused) {
      if ((rc = eval_tiles(e, e->stream, false, false))) return rc;
      own_launch = true;
    }
    if (fused) job->fused_pending = false;
    {  // alpha = U v of the launch, refined against L (intact, diagonal tiles in place) before the a a^T term reads it
      const TriOperand L{e->dA, e->ld, e->dA, e->ld, (int64_t)TILE * (e->ld + 1)};
      const TriOperand U{e->dA, e->ld, e->dUdiag, TILE, (int64_t)TILE * TILE};
      if ((rc = refine_alpha(e, L, &U, nullptr, 0))) return rc;
    }
    if ((rc = grad_reduce(e, 0, 1, e->dW, e->Np, false, h, GradLanding{light, light}))) return rc;  // (light: its clear covered the accumulators)
    if (tgt) tgt->stop();
    uint32_t ab = 0;
    if (own_launch) HIP_TRY(e, hipMemcpyAsync(&ab, e->dct + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    if (tgt) tm.grad_ms = tgt->ms();
    ev_collect(e);
    if (light) {
      for (size_t t = 0; t < e->terms.size(); ++t)
        std::copy(e->hl->gacc + t * GACC_REGION, e->hl->gacc + (t + 1) * GACC_REGION, h.begin() + t * GACC_REGION);
      e->fs.gradient_left_u_and_alpha();  // (gmb_evaluate takes both back if factorize_finish reports a failure)
      return GMB_OK;  // (abort word, failure index: factorize_finish, which gmb_evaluate calls next)
    }
    if (ab != 0) return fail(e, GMB_EHIP, "tile inverse: a workgroup waited longer than its time-out for a tile (launch abandoned)");
    e->fs.gradient_left_u_and_alpha();
    return GMB_OK;
  }
  if ((rc = e->dDiagSave.reserve(e->pool, (int64_t)nt * TILE * TILE))) return rc;
  e->fs.inverse_rewrites_u();
  PhaseTimer tg(e);
  // 0. + 1. W = L^-1 (dW, lower) and U = L^-T (factor buffer, upper); the factor is consumed from here on
  e->fs.consume();
  if ((rc = tri_inverse_pair(e, job && job->in_flight))) return rc;
  // 2. alpha = W^T v = Sigma^-1 y   (before Sigma^-1 overwrites W)
  hipLaunchKernelGGL(wt_v_kernel, dim3((unsigned)((e->N + 3) / 4)), dim3(256), 0, e->stream, e->dW, e->Np,
                     e->dv, e->N, e->dalpha);
  {  // ... refined against L (its diagonal blocks wait in dDiagSave while U's sit in the factor buffer)
    const TriOperand L{e->dA, e->ld, e->dDiagSave, TILE, (int64_t)TILE * TILE};
    if ((rc = refine_alpha(e, L, nullptr, e->dW, e->Np))) return rc;
  }
  // 3. Sigma^-1 = U U^T (lower triangle) into dW -- the last reader of U: the factor's diagonal blocks go back
  if ((rc = inverse_from_pair(e))) return rc;
  // 4. fused trace reductions
  if ((rc = grad_reduce(e, 0, 1, e->dW, e->Np, false, h, GradLanding{}))) return rc;
  tg.stop();
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  tm.grad_ms = tg.ms();
  ev_collect(e);
  e->fs.restore();  // lower triangle = L again (the upper triangle keeps U: scratch as far as L goes)
  return GMB_OK;
}

// Host part: chain rule from the (summed) accumulators back to the packed natural-scale parameters.
int grad_chain_rule(gmb_engine* e, const std::vector<double>& h, double* grad) {
  const gmb_kernel_spec& s = e->spec;
  const int n_ls = s.ard ? s.n_cont : 1;
  const double* th = e->theta.data();
  auto region = [&](size_t t) { return h.data() + t * GACC_REGION; };
  auto table_slot = [&](size_t t, int j) {  // j-th table of term t inside its region
    int off = 64;
    for (int q = 0; q < j; ++q) off += e->terms[t].cp.tab_levels[q] * e->terms[t].cp.tab_levels[q];
    return region(t) + off;
  };
  auto kernel_block = [&](size_t t, double* g) {  // [ls | eta] and, after a gap the caller fills, [c | tau]
    const double* r = region(t);
    int k = 0;
    for (int i = 0; i < n_ls; ++i) g[k++] = r[i];
    g[k++] = r[n_ls];
    return k;
  };
  auto table_grad = [&](const std::vector<double>& G, int L, const double* W, double* g) {
    for (int x = 0; x < L; ++x)
      for (int q = 0; q < 2; ++q) {
        double acc = 0.0;
        for (int b = 0; b < L; ++b) acc += (G[x * L + b] + G[b * L + x]) * W[2 * b + q];
        g[2 * x + q] = acc;
      }
    for (int x = 0; x < L; ++x) g[2 * L + x] = G[x * L + x];
  };
  // global term: ls | eta | sigma | c | tau
  int k = kernel_block(0, grad);
  const int i_sigma = k++;
  if (s.n_lin > 0) {
    for (int i = 0; i < s.n_lin; ++i) grad[k++] = region(0)[n_ls + 2 + i];
    grad[k++] = region(0)[n_ls + 1];  // tau
  }
  // coregion tables of the categorical dims, then the output table
  const int ntab = spec_ntab(s);
  for (int j = 0; j < ntab; ++j) {
    const bool is_out = (j == s.n_coreg);
    const int L = is_out ? s.n_out : s.coreg_levels[j];
    std::vector<double> G((size_t)L * L, 0.0);
    if (!s.additive) {
      const double* src = table_slot(0, j);
      for (int i = 0; i < L * L; ++i) G[i] = src[i];
    } else if (!is_out) {
      const double* src = table_slot(1 + j, 0);  // the dim's own term carries its table first
      for (int i = 0; i < L * L; ++i) G[i] = src[i];
    } else {
      for (size_t t = 0; t < e->terms.size(); ++t) {  // every term is multiplied by the output table
        const double* src = table_slot(t, e->terms[t].cp.n_tab - 1);
        for (int i = 0; i < L * L; ++i) G[i] += src[i];
      }
    }
    table_grad(G, L, th + k, grad + k);
    k += 3 * L;
  }
  // noise: region 0 keeps [sigma, noise table ...] after the global term's tables
  int diag_off = 64;
  for (int j = 0; j < e->terms[0].cp.n_tab; ++j) diag_off += e->terms[0].cp.tab_levels[j] * e->terms[0].cp.tab_levels[j];
  const double* hd = region(0) + diag_off;
  grad[i_sigma] = hd[0];
  if (s.out_col >= 0 && s.hetero_noise) {
    const int P = s.n_out;
    const double* W = th + k;
    for (int x = 0; x < P; ++x) {
      const double gd = hd[1 + x];
      grad[k + 2 * x] = 2.0 * gd * W[2 * x];
      grad[k + 2 * x + 1] = 2.0 * gd * W[2 * x + 1];
      grad[k + 2 * P + x] = gd;
    }
    k += 3 * P;
  }
  // additive terms: ls | eta | c | tau per coregion dim
  if (s.additive)
    for (int j = 0; j < s.n_coreg; ++j) {
      k += kernel_block(1 + j, grad + k);
      if (s.n_lin > 0) {
        for (int i = 0; i < s.n_lin; ++i) grad[k++] = region(1 + j)[n_ls + 2 + i];
        grad[k++] = region(1 + j)[n_ls + 1];
      }
    }
  if (k != (int)e->theta.size()) return fail(e, GMB_EINVAL, "internal: gradient packing mismatch");
  return GMB_OK;
}

// -1 = by size (default), 0 = plain recursion, 2 = masked look-ahead streams, 3 = persistent tile kernel
inline bool chol_scheme_valid(int s) { return s == -1 || s == 0 || s == 2 || s == 3 || s == 4; }

int require_ready(gmb_engine* e, bool need_factor) {
  if (!e) return GMB_EINVAL;
  if (e->N <= 0) return fail(e, GMB_EINVAL, "gmb_set_data has not been called");
  if (!e->have_spec) return fail(e, GMB_EINVAL, "gmb_set_kernel has not been called");
  if (!e->have_theta) return fail(e, GMB_EINVAL, "gmb_set_theta has not been called");
  if (need_factor && !e->fs.valid())
    return fail(e, GMB_EINVAL, "no valid factorisation: call gmb_factorize first");
  return GMB_OK;
}

// The calls that read the COMPLETE factor out of dA (single-engine gradient / prediction / factor windows, the replicated
// multi-GPU passes) against a factorisation of the capacity driver, which leaves none there -- and the reverse: the capacity
// passes against anything else than a capacity factorisation (their dAown would be an older theta's).
int require_full_factor(gmb_engine* e, const char* what) {
  if (e->fs.capacity() || !e->dA || e->dA.cap <= 0)
    return fail(e, GMB_EINVAL, "%s needs the complete factor on this device, but the resident factorisation is a capacity-mode one "
                               "(gmb_dist_set_mode(e, 1): no rank holds the factor) -- use the gmb_dist_* calls, or gmb_factorize first", what);
  return GMB_OK;
}

int require_capacity_factor(gmb_engine* e, const char* what) {
  if (!e->fs.capacity() || !e->dAown)
    return fail(e, GMB_EINVAL, "%s in capacity mode needs a factorisation made by gmb_dist_factorize in capacity mode; the resident "
                               "one was made by %s", what, e->fs.single() ? "gmb_factorize / gmb_evaluate" : "the replicated multi-GPU driver");
  return GMB_OK;
}

}  // namespace

namespace {

// ONE CU-masked bulk stream per process and device, created on first use and never destroyed (masked
// streams that were created and destroyed with every engine made kernel timings depend on the queue
// history of the process).  It leaves `part_cus / 8` compute units of every XCD free for the latency-bound
// panel chain of chol_lookahead_masked; the runtime applies a CU mask symmetrically to all XCDs (bit i <->
// XCD i % 8, compute unit i / 8 of it -- tools/probes/cumask_probe.hip).  Engines on one device share it,
// i.e. their trailing updates serialise on it; every engine joins it back into its own stream before
// gmb_factorize returns.
hipStream_t shared_masked_stream(int device, int part_cus, int* ncu_out) {
  static std::mutex mu;
  static hipStream_t streams[64] = {};
  static int ncus[64] = {};
  std::lock_guard<std::mutex> lock(mu);
  hipStream_t& st = streams[device & 63];
  if (!st) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return nullptr;
    const int ncu = prop.multiProcessorCount;
    std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
    for (int i = part_cus; i < ncu; ++i) mask[i / 32] |= 1u << (i % 32);
    if (hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
      st = nullptr;
      (void)hipGetLastError();
      return nullptr;
    }
    ncus[device & 63] = ncu;
  }
  if (ncu_out) *ncu_out = ncus[device & 63];
  return st;
}

int gmb_create_impl(gmb_engine** out, int32_t device, void* stream, const gmb_engine* peer = nullptr) {
  if (!out) return GMB_EINVAL;
  *out = nullptr;
  int n = gmb_device_count();
  if (n < 0) return GMB_ENODEVICE;
  if (device < 0 || device >= n) return GMB_EINVAL;
  if (hipSetDevice(device) != hipSuccess) return GMB_EHIP;
  gmb_engine* e = new gmb_engine();
  e->device = device;
  if (stream) {
    e->stream = (hipStream_t)stream;
  } else {
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) {
      delete e;
      return GMB_EHIP;
    }
    e->own_stream = true;
  }
  auto flag = [](const char* name, bool dflt) {
    const char* v = getenv(name);
    return v && v[0] ? v[0] != '0' : dflt;
  };
  // Environment switches of the PRODUCT library: only the ones a test or a documented tools/ A-B uses.
  //   GMB_LEAF_NAIVE=1   the reference diagonal-block kernel (tests/test_gpu_parity.py::test_potrf_leaf_block)
  //   GMB_CHOL_SCHEME    0 = plain recursion (launches only), 2 = masked look-ahead, 3 = persistent tile kernel, 4 = plain recursion
  //                      with its bottom panels on the tile kernel (what large matrices take by size), for every size
  //                      (tests/test_gpu_parity.py::test_cholesky_schedules_agree); default: by size
  //   GMB_TRACE_FILE     per-launch event log while profiling (tools/gpu_timeline_run.py)
  //   GMB_GEMM_DMA=0     the 128 x 128 GEMM with register staging instead of the LDS-DMA ring (tools/gpu_ab_gemm_dma.py)
  // Everything else is compiled in only with -DGMB_TUNING (GUMBI_BUILD_TUNING=1 python -m gumbi_amd.build writes
  // gumbi_amd/lib/libgumbi_hip_tuning.so; tools/README.md).
  e->naive_leaf = flag("GMB_LEAF_NAIVE", false);
  e->gemm_dma = flag("GMB_GEMM_DMA", true);
  const char* cs = getenv("GMB_CHOL_SCHEME");
  if (cs && cs[0]) {
    const int v = atoi(cs);
    if (chol_scheme_valid(v)) e->chol_scheme = v;
    else fprintf(stderr, "[gumbi_hip] GMB_CHOL_SCHEME=%s ignored: valid schemes are -1 (by size), 0, 2, 3, 4\n", cs);
  }
  int part = 32;  // compute units the masked bulk stream leaves to the panel chain
#ifdef GMB_TUNING
  e->small_tiles = flag("GMB_SMALL_TILES", true);
  const char* gv = getenv("GMB_GEMM_VARIANT");  // pins the tile shape of every out-of-place GEMM: 0 .. 3
  if (gv && gv[0] >= '0' && gv[0] <= '4') {
    e->gemm_variant = gv[0] - '0';
    e->force_variant = true;
  }
  e->lookahead = flag("GMB_LOOKAHEAD", true);
  e->lpt_order = flag("GMB_LPT_ORDER", true);
  if (const char* lm = getenv("GMB_LPT_MAX_TILES")) e->lpt_max_tiles = atoll(lm);
  const char* ts = getenv("GMB_TILE_STRIP");
  if (ts) e->tile_strip = std::max(0, atoi(ts));
  const char* cst = getenv("GMB_COV_STRIP");
  if (cst) e->cov_strip = std::max(0, std::min(64, atoi(cst)));
  e->batch_inverse = flag("GMB_BATCH_INVERSE", true);
  e->par_inverse = flag("GMB_PAR_INVERSE", true);
  const char* pb = getenv("GMB_PANEL_BLOCKS");
  if (pb && atoi(pb) > 0) {
    e->panel_blocks = atoi(pb);
    e->panel_auto = false;
  }
  const char* mb = getenv("GMB_MASKED_MAX_BLOCKS");
  if (mb) e->masked_max_blocks = atoi(mb);
  if (const char* pw = getenv("GMB_PANEL_TILES_W")) e->panel_tiles_w = std::max(0, std::min(64, atoi(pw)));  // (tools/gpu_panel_tiles_ab.py)
  const char* pc = getenv("GMB_PART_CUS");
  if (pc) part = atoi(pc);
#endif
  // Exactly four streams per engine (beyond four hardware queues the runtime multiplexes streams and every
  // kernel of the process slows down -- measured): the caller's, aux[0] / aux[1] at the highest queue
  // priority (panel chain of the unmasked look-ahead; independent merges of the triangular inverse), and
  // aux[2] = the bulk stream of the trailing updates: the process-wide CU-masked stream (GMB_PART_CUS
  // compute units left free, default 32; tuning builds: 0 = an ordinary lowest-priority stream).
  int prio_lo = 0, prio_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  for (int a = 0; a < 3 && peer; ++a) {  // sibling: the peer's streams (its engines work one after the other)
    e->aux[a] = peer->aux[a];
    e->aux_borrowed = true;
    e->aux_shared = peer->aux_shared;
    e->part_cus = peer->part_cus;
  }
  for (int a = 0; a < 3 && !peer; ++a) {
    hipError_t st2 = hipSuccess;
    int ncu = 0;
    hipStream_t masked = (a == 2 && part > 0) ? shared_masked_stream(device, part, &ncu) : nullptr;
    if (masked) {
      e->aux[a] = masked;
      e->aux_shared = true;
      e->part_cus = part;
    } else {
      st2 = hipStreamCreateWithPriority(&e->aux[a], hipStreamNonBlocking, a == 2 ? prio_lo : prio_hi);
    }
    if (st2 != hipSuccess) {
      gmb_destroy(e);
      return GMB_EHIP;
    }
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) e->wg_slots = 2LL * prop.multiProcessorCount;
  e->pool.owner = e;
  e->pool.refused = alloc_refused;
  // (uncounted: fixed overhead of every engine, not what gmb_resident_bytes reports)
  if (e->dscal.renew(e->pool, SCAL_DOUBLES, false) || e->dstat.renew(e->pool, (DIST_HEADER + DIST_MAX_PAYLOAD) * (1 + DIST_MAX_WORLD), false)) {
    gmb_destroy(e);
    return GMB_ENOMEM;
  }
  e->dinfo = reinterpret_cast<int32_t*>(e->dscal + SCAL_INFO_AT);
  e->dgpart = e->dscal + SCAL_GACC_AT;
  *out = e;
  return GMB_OK;
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

int gmb_abi_version(void) { return GMB_ABI_VERSION; }

int gmb_device_count(void) {
  int n = 0;
  hipError_t s = hipGetDeviceCount(&n);
  if (s != hipSuccess || n <= 0) return GMB_ENODEVICE;
  return n;
}

int gmb_create(gmb_engine** out, int32_t device, void* stream) { return gmb_create_impl(out, device, stream); }

int gmb_create_sibling(gmb_engine** out, const gmb_engine* peer) {
  if (!peer) return GMB_EINVAL;
  return gmb_create_impl(out, peer->device, (void*)peer->stream, peer);
}

void gmb_destroy(gmb_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  // the engine's own work on every stream it used (the shared bulk stream is joined into e->stream at the
  // end of every factorisation, but an error return may have skipped that)
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  for (int a = 0; a < 3; ++a)
    if (e->aux[a]) (void)hipStreamSynchronize(e->aux[a]);
  e->pool.release_all();
  for (int a = 0; a < 3; ++a)
    if (e->aux[a] && !e->aux_borrowed && !(a == 2 && e->aux_shared)) (void)hipStreamDestroy(e->aux[a]);
  for (auto ev : e->fe)
    if (ev) (void)hipEventDestroy(ev);
  if (e->hl) (void)hipHostFree(e->hl);
  for (auto ev : e->sync_pool) (void)hipEventDestroy(ev);
  for (auto ev : e->time_pool) (void)hipEventDestroy(ev);
  if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

const char* gmb_last_error(const gmb_engine* e) { return e ? e->err.c_str() : "null engine"; }
void* gmb_stream(const gmb_engine* e) { return e ? (void*)e->stream : nullptr; }

int gmb_theta_size(const gmb_kernel_spec* s) {
  if (!s) return GMB_EINVAL;
  int n = (s->ard ? s->n_cont : 1) + 2;
  if (s->n_lin > 0) n += s->n_lin + 1;
  for (int t = 0; t < s->n_coreg; ++t) n += 3 * s->coreg_levels[t];
  if (s->out_col >= 0) {
    n += 3 * s->n_out;
    if (s->hetero_noise) n += 3 * s->n_out;
  }
  if (s->additive) {
    const int blk = (s->ard ? s->n_cont : 1) + 1 + (s->n_lin > 0 ? s->n_lin + 1 : 0);
    n += s->n_coreg * blk;
  }
  return n;
}

int gmb_set_data(gmb_engine* e, const double* X, int64_t N, int32_t D, int64_t ldx, const double* y,
                 int32_t memspace) {
  if (!e) return GMB_EINVAL;
  if (!X || !y || N < 1 || D < 1 || ldx < D) return fail(e, GMB_EINVAL, "bad X/y/N/D/ldx");
  if (e->have_spec) {
    int rc = validate_spec(e, e->spec, D);
    if (rc) return rc;
  }
  HIP_TRY(e, hipSetDevice(e->device));
  // not ready until every allocation below has succeeded; workspaces sized for the previous N / D are dropped
  e->fs.feature_map_changed();  // (no factorisation of THIS data has been attempted: gmb_debug_assume_factored must refuse)
  e->have_theta = false;
  e->N = 0;
  e->fitc.drop_inducing();
  e->lap.drop("gmb_set_data changed the data");
  stale_sized_by_n(e);
  // (here only: new data gets prepared points of exactly its own size.  resize_n keeps a block that is large enough -- after
  // a truncation it is larger than Nr asks for, and renewing it there would move gmb_resident_bytes.)
  e->pts.stale();
  e->D = D;
  e->Np = round_up(N, TILE);
  e->Nr = round_up(N + 1, TILE);
  e->ld = e->Nr;
#ifdef GMB_TUNING
  if (const char* lp = getenv("GMB_LD_PAD")) e->ld = e->Nr + atoi(lp);  // probe: leading dimension off the 1 KiB grid (tools/gpu_ld_pad.py)
#endif
  int rc;
  if ((rc = e->dX.renew(e->pool, N * (int64_t)D))) return rc;
  if ((rc = e->dy.renew(e->pool, e->Np))) return rc;
  // (the factor buffer itself -- Nr x Np doubles -- is allocated by the first factorisation that needs it: in the multi-GPU
  // driver's capacity mode no rank ever holds it)
  if (e->dA.cap < e->ld * e->Np) e->dA.drop(e->pool);
  if ((rc = e->dDinv16.reserve(e->pool, (e->Np / TILE) * (int64_t)8 * 256))) return rc;
  if ((rc = e->dv.renew(e->pool, e->Np))) return rc;
  const hipMemcpyKind kind = memspace == GMB_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIP_TRY(e, hipMemcpy2DAsync(e->dX, D * sizeof(double), X, ldx * sizeof(double), D * sizeof(double), N,
                              kind, e->stream));
  HIP_TRY(e, hipMemsetAsync(e->dy, 0, e->Np * sizeof(double), e->stream));
  HIP_TRY(e, hipMemcpyAsync(e->dy, y, N * sizeof(double), kind, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  e->N = N;
  return GMB_OK;
}

int gmb_set_y(gmb_engine* e, const double* y, int32_t memspace) {
  if (!e) return GMB_EINVAL;
  if (e->N <= 0) return fail(e, GMB_EINVAL, "gmb_set_data must precede gmb_set_y");
  if (!y) return fail(e, GMB_EINVAL, "y is null");
  HIP_TRY(e, hipSetDevice(e->device));
  const hipMemcpyKind kind = memspace == GMB_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  e->fs.inputs_changed();  // the y row of the factor (v = L^-1 y) belongs to the old observations
  e->fitc.resident = false;
  e->lap.drop("gmb_set_y changed the labels");
  HIP_TRY(e, hipMemcpyAsync(e->dy, y, e->N * sizeof(double), kind, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));  // the caller may reuse its buffer
  return GMB_OK;
}

int gmb_set_kernel(gmb_engine* e, const gmb_kernel_spec* spec) {
  if (!e || !spec) return GMB_EINVAL;
  int rc = validate_spec(e, *spec, e->D);
  if (rc) return rc;
  e->spec = *spec;
  e->have_spec = true;
  e->have_theta = false;
  e->fs.inputs_changed();
  e->fitc.drop_inducing();
  e->lap.drop("gmb_set_kernel changed the kernel");
  e->nc_pad = pick_nc(spec->n_cont);
  e->periodic = 0;
  e->pts.stale();
  return GMB_OK;
}

int gmb_set_periodic(gmb_engine* e, int32_t mode, const double* periods, int32_t n) {
  if (!e) return GMB_EINVAL;
  if (!e->have_spec) return fail(e, GMB_EINVAL, "gmb_set_kernel must precede gmb_set_periodic");
  const gmb_kernel_spec& s = e->spec;
  if (mode < 0 || mode > 2) return fail(e, GMB_EINVAL, "gmb_set_periodic: mode %d must be 0 (off), 1 (<kind>+Periodic) or 2 (Periodic)", mode);
  if (n != s.n_cont) return fail(e, GMB_EINVAL, "gmb_set_periodic: %d periods for %d continuous dimensions", n, s.n_cont);
  if (mode != 0) {
    if (s.n_cont > GMB_MAX_DIMS / 2)
      return fail(e, GMB_EINVAL, "gmb_set_periodic: a periodic model has at most %d continuous dimensions (two prepared columns each), got %d",
                  GMB_MAX_DIMS / 2, s.n_cont);
    if (mode == 2 && s.kind != GMB_EXPQUAD) return fail(e, GMB_EINVAL, "gmb_set_periodic: mode 2 (Periodic) needs kind ExpQuad, got %d", s.kind);
    if (!periods) return fail(e, GMB_EINVAL, "gmb_set_periodic: periods is null");
    for (int i = 0; i < n; ++i)
      if (!std::isfinite(periods[i]) || !(periods[i] > 0.0))
        return fail(e, GMB_EINVAL, "gmb_set_periodic: period %d = %g must be finite and positive", i, periods[i]);
  }
  e->periodic = mode;
  for (int i = 0; i < 8; ++i) e->periods[i] = (mode != 0 && i < n) ? periods[i] : 0.0;
  e->nc_pad = pick_nc(mode != 0 ? 2 * s.n_cont : s.n_cont);
  // the prepared coordinates and everything factored from them belong to the previous feature map
  e->have_theta = false;
  e->fs.feature_map_changed();
  e->fitc.drop_inducing();
  e->lap.drop("gmb_set_periodic changed the kernel");
  return GMB_OK;
}

// gmb_set_theta; inside a gmb_evaluate, `plan` says what the preparation of the points clears and whether it is left to the
// covariance build
static int set_theta(gmb_engine* e, const double* theta, int32_t n, const EvalPlan* plan) {
  if (!e || !theta) return GMB_EINVAL;
  if (!e->have_spec) return fail(e, GMB_EINVAL, "gmb_set_kernel must precede gmb_set_theta");
  if (e->N <= 0) return fail(e, GMB_EINVAL, "gmb_set_data must precede gmb_set_theta");
  if (n != gmb_theta_size(&e->spec))
    return fail(e, GMB_EINVAL, "theta has %d entries, kernel needs %d", n, gmb_theta_size(&e->spec));
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(theta[i])) return fail(e, GMB_EINVAL, "theta[%d] is not finite", i);
  HIP_TRY(e, hipSetDevice(e->device));
  e->theta.assign(theta, theta + n);
  e->fs.inputs_changed();
  e->fitc.resident = false;  // (Lu, L_B, c belong to the previous theta)
  e->lap.drop("theta was set again (gmb_set_theta, gmb_evaluate, gmb_fitc_evaluate)");
  int rc = apply_theta(e);
  if (rc) return rc;
  if ((rc = e->pts.reserve(e->pool, e->Nr))) return rc;
  PrepClears clears;
  if (plan && plan->prezero) {
    // gmb_evaluate: this launch also clears the scalar block and the tile launch's control words (factorize_enqueue, eval_tiles)
    if ((rc = e->dct.reserve(e->pool, eval_tiles_words((int)(e->Np / TILE), (int)(e->Nr / TILE)) + 2))) return rc;
    clears = eval_clears(e);
  }
  // small evaluations: the covariance build of this same gmb_evaluate prepares the points itself (one launch less)
  if (!(plan && plan->inline_prep) && (rc = prep_points(e, e->dX, e->N, e->D, e->Nr, e->pts.xs, e->pts.xl, e->pts.cat, nullptr, clears))) return rc;
  e->have_theta = true;
  return GMB_OK;
}

int gmb_set_theta(gmb_engine* e, const double* theta, int32_t n) { return set_theta(e, theta, n, nullptr); }

int gmb_set_profiling(gmb_engine* e, int32_t on) {
  if (!e) return GMB_EINVAL;
  e->profiling = on != 0;
  if (on) {
    e->tm.total_gemm_ms = e->tm.total_gemm_flops = 0.0;
    e->tm.masked_gemm_ms = e->tm.masked_gemm_flops = 0.0;
    e->tm.total_gemm_wall_ms = 0.0;
    e->tm.total_chol_gemm_ms = e->tm.total_chol_gemm_flops = e->tm.total_chol_gemm_wall_ms = 0.0;
    e->tm.total_chol_gemm_launches = 0;
    e->tm.total_chol_panel_gemm_ms = e->tm.total_chol_panel_gemm_flops = 0.0;
    e->tm.total_chol_tile_ms = e->tm.total_chol_tile_flops = 0.0;
    e->tm.total_chol_tile_launches = 0;
    e->tm.total_chol_update_all_ms = e->tm.total_chol_update_all_flops = 0.0;
    e->tm.total_chol_update_all_launches = 0;
    e->tm.total_chol_panel_tile_ms = e->tm.total_chol_panel_tile_flops = 0.0;
    e->tm.total_chol_panel_tile_launches = 0;
    e->tm.masked_cus = e->aux_shared ? e->wg_slots / 2 - e->part_cus : 0;
    e->tm.total_gemm_launches = 0;
    e->tm.total_kbuild_ms = e->tm.total_kbuild_bytes = 0.0;
    e->tm.total_kbuild_launches = 0;
  }
  return GMB_OK;
}

int gmb_timings_get(const gmb_engine* e, gmb_timings* out) {
  if (!e || !out) return GMB_EINVAL;
  *out = e->tm;
  return GMB_OK;
}

int64_t gmb_notpd_index(const gmb_engine* e) { return e ? e->notpd : -1; }

int gmb_factor_valid(const gmb_engine* e) { return (e && e->N > 0 && e->have_theta && e->fs.usable()) ? 1 : 0; }

namespace {

// What every factorisation does first -- gmb_factorize / gmb_evaluate, the two multi-GPU drivers and (`tail`) the bordered update
// behind gmb_append / gmb_truncate: nothing of the previous one stays valid, no failure index, the phase timings start from zero.
void begin_factorisation(gmb_engine* e, FactorState::Kind kind, bool tail = false) {
  tail ? e->fs.begin_tail() : e->fs.begin(kind);
  e->lap.drop("a factorisation of Sigma (gmb_factorize, gmb_evaluate, gmb_dist_*) took the factor buffer");  // (B's factor sat there)
  e->notpd = -1;
  gmb_timings& tm = e->tm;
  tm.kbuild_ms = tm.chol_ms = tm.chol_gemm_ms = tm.chol_gemm_flops = tm.chol_leaf_ms = tm.chol_trsm_ms = 0.0;
  tm.chol_gemm_launches = 0;
}

// ... and what every one of them does last, with the failure index, log-det and |v|^2 its host has read
int accept_factor(gmb_engine* e, int32_t info, double logdet, double vnorm2) {
  if (info != 0) {
    e->notpd = (int64_t)info - 1;
    return fail(e, GMB_ENOTPD, "covariance matrix is not positive definite at row %lld", (long long)e->notpd);
  }
  e->logdet = logdet;
  e->vnorm2 = vnorm2;
  if (!std::isfinite(e->logdet) || !std::isfinite(e->vnorm2)) {
    e->notpd = 0;
    return fail(e, GMB_ENOTPD, "factorisation produced non-finite values");
  }
  e->fs.accepted();
  return GMB_OK;
}

// the events around the covariance build and the Cholesky (kbuild_ms, chol_ms)
int ensure_phase_events(gmb_engine* e) {
  for (auto& ev : e->fe)
    if (!ev) HIP_TRY(e, hipEventCreate(&ev));
  return GMB_OK;
}

// the pinned block the factorisation's scalars land in, with no failure and no abandoned launch on record
int ensure_host_landing(gmb_engine* e) {
  if (!e->hl) {
    HIP_TRY(e, hipHostMalloc((void**)&e->hl, sizeof(gmb_engine::HostLanding), hipHostMallocDefault));
    HIP_TRY(e, hipHostGetDevicePointer((void**)&e->hl_dev, e->hl, 0));
  }
  e->hl->info = 0;
  e->hl->abort = 0;
  return GMB_OK;
}

// Everything of gmb_factorize up to (not including) the host's look at the results: K-build, Cholesky, v = L^-1 y, and the
// asynchronous copies of log-det / |v|^2 / failure index / abort word into the engine.  Nothing is synchronised.
int factorize_enqueue(gmb_engine* e, FactorJob& job) {
  const auto [light, prezero, inline_prep, events] = job.plan;
  int rc = require_ready(e, false);
  if (rc) return rc;
  HIP_TRY(e, hipSetDevice(e->device));
  begin_factorisation(e, FactorState::SINGLE);
  if ((rc = ensure_factor_buffer(e))) return rc;
  if ((rc = ensure_phase_events(e))) return rc;
  if (e->panel_auto) {
    // wider panels for larger matrices: a k = 1024 trailing update pays its C read-modify-write and
    // epilogue per 1024 of contraction; measured at N = 60k: 8 blocks 58.0, 16: 62.2, 32: 63.9 TF/s
    // (N = 10k: 4 .. 16 within 2 %)
    const int nct = (int)(e->Np / TILE);
    e->panel_blocks = std::max(8, ((nct / 16 + 4) / 8) * 8);
  }
  // the fused evaluation launch pays at every size (per evaluation, stream schedules -> fused: N = 100: 0.21 -> 0.14 ms, N = 392:
  // 0.44 -> 0.27, N = 1000: 0.76 -> 0.45; tools/gpu_small_eval.py), the tile Cholesky on its own only from six block columns:
  // a `light` plan is gmb_evaluate on that launch, and everything the host wants lands through eval_land_kernel at the end of the gradient
  job.events_recorded = events;
  // scalars + failure index (+ the gradient's accumulators): one memset -- or none, when the evaluation's preparation launch
  // clears them (`prezero`)
  if (!prezero) HIP_TRY(e, hipMemsetAsync(e->dscal, 0, (size_t)(light ? SCAL_DOUBLES : SCAL_GACC_AT) * sizeof(double), e->stream));

  // 1. covariance build: lower-triangular tiles of Sigma, y row, identity padding
  if (events) HIP_TRY(e, hipEventRecord(e->fe[0], e->stream));
  job.build_reached = true;
  const PrepClears clears = inline_prep ? eval_clears(e) : PrepClears{};
  if ((rc = build_sigma(e, e->dA, e->ld, inline_prep ? &clears : nullptr))) return rc;
  if (events) HIP_TRY(e, hipEventRecord(e->fe[1], e->stream));
  // 2. Cholesky
  if (events) HIP_TRY(e, hipEventRecord(e->fe[2], e->stream));
  e->chol = CholResult{};
  if (light) {
    // the gradient's inverse and Sigma^-1 ride in the factorisation's launch (eval_tiles.hpp); v = L^-1 y (row N of the factor)
    // and |v|^2 come out of the launch that adds up alpha
    if ((rc = eval_tiles(e, e->stream, true, prezero))) return rc;
    job.fused_pending = true;
  } else {
    CholOpts o;
    o.masked_ok = true;
    o.trace = e->ct_trace;
    o.lose = e->ct_lose;
    rc = chol_factor(e, train_factor(e), o, &e->chol);
    if (e->chol.injected) e->ct_lose = 0;  // (one shot)
    if (rc) return rc;
    // 3. v = L^-1 y is row N of the factor
    hipLaunchKernelGGL(extract_v_kernel, dim3(EXTRACT_V_BLOCKS), dim3(TILE), 0, e->stream, e->dA, e->ld, e->N, e->dv,
                       e->dscal + 1);
  }
  if (events) HIP_TRY(e, hipEventRecord(e->fe[3], e->stream));
  HIP_TRY(e, hipGetLastError());
  if ((rc = ensure_host_landing(e))) return rc;
  if (!light) {
    HIP_TRY(e, hipMemcpyAsync(e->hl->scal, e->dscal, 2 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipMemcpyAsync(&e->hl->info, e->dinfo, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (e->chol.tiles) HIP_TRY(e, hipMemcpyAsync(&e->hl->abort, e->dct + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  }
  job.in_flight = true;
  return GMB_OK;
}

// The host's look at an enqueued factorisation: synchronise, timings, failure checks; accepts the factor or not.
int factorize_finish(gmb_engine* e, FactorJob& job) {
  gmb_timings& tm = e->tm;
  e->fs.not_accepted();
  job.in_flight = false;
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  if (!e->hl) return fail(e, GMB_EINVAL, "internal: no factorisation enqueued");
  if (e->hl->abort != 0) {
    ev_collect(e);
    return fail(e, GMB_EHIP, "tile Cholesky: a workgroup waited longer than its time-out for a tile (launch abandoned)");
  }
  float t = 0.f;
  if (job.events_recorded && hipEventElapsedTime(&t, e->fe[0], e->fe[1]) == hipSuccess) tm.kbuild_ms = t;
  if (job.events_recorded && hipEventElapsedTime(&t, e->fe[2], e->fe[3]) == hipSuccess) tm.chol_ms = t;
  tm.kbuild_bytes = 8.0 * (double)e->N * (double)(e->N + 1) / 2.0 +
                    8.0 * (double)e->N * (double)(e->spec.n_cont + 1);
  ev_collect(e);
  if (e->profiling) {
    tm.total_kbuild_ms += tm.kbuild_ms;
    tm.total_kbuild_bytes += tm.kbuild_bytes;
    tm.total_kbuild_launches += 1;
  }
  return accept_factor(e, e->hl->info, e->hl->scal[0], e->hl->scal[1]);
}

}  // namespace

// A tile-kernel launch that gave up waiting (abort word set: a lost flag, or a GPU shared with a process that starved it
// for seconds) says nothing about the matrix: factor it once more with the plain recursion before reporting an error.
// Injected faults (gmb_debug_chol_lose_tickets) are reported as they are -- the tests want to see the bounded wait.
static int factorize_retry_after_abort(gmb_engine* e, int rc) {
  if (rc != GMB_EHIP || !e->chol.tiles || !e->hl || e->hl->abort == 0 || e->chol.injected) return rc;
  fprintf(stderr, "libgumbi_hip: tile Cholesky abandoned after a time-out; refactorising with the plain recursion\n");
  const int scheme = e->chol_scheme;
  e->chol_scheme = 0;  // (scheme 0 = launches only: no tile kernel anywhere, the recursion's bottom panels included)
  FactorJob job;  // (a fresh plain one)
  int rc2 = factorize_enqueue(e, job);
  if (!rc2) rc2 = factorize_finish(e, job);
  e->chol_scheme = scheme;
  return rc2;
}

int gmb_factorize(gmb_engine* e) {
  FactorJob job;
  int rc = factorize_enqueue(e, job);
  if (!rc) rc = factorize_retry_after_abort(e, factorize_finish(e, job));
  return rc;
}

int gmb_evaluate(gmb_engine* e, const double* theta, int32_t n, double* nlml, double* grad) {
  if (!e || !nlml) return GMB_EINVAL;
  FactorJob job;
  job.plan = plan_evaluate_call(e, grad != nullptr);
  int rc = set_theta(e, theta, n, &job.plan);
  if (rc) return rc;
  rc = factorize_enqueue(e, job);
  if (job.plan.inline_prep && !job.build_reached) {
    // the covariance build was not reached (an allocation failed): the points are prepared now -- without the plan's clears:
    // nothing reads those words before the next factorisation clears them itself
    const int rc2 = prep_points(e, e->dX, e->N, e->D, e->Nr, e->pts.xs, e->pts.xl, e->pts.cat);
    if (!rc) rc = rc2;
  }
  if (rc) return rc;
  int rc_grad = GMB_OK;
  std::vector<double> h;
  if (grad) {
    // the gradient's launches follow the factorisation's on the same stream with no host round trip in between; if the
    // factorisation turns out to have failed they ran on garbage and their result is dropped below
    e->fs.accepted();
    const bool fused = job.fused_pending;  // (a light plan: the factorisation's results land with the gradient's)
    rc_grad = grad_accumulate(e, h, &job);
    if (rc_grad && fused) {  // nothing has landed on the host: there is no factorisation to look at
      (void)hipStreamSynchronize(e->stream);
      e->fs.not_accepted();
      return rc_grad;
    }
  }
  if ((rc = factorize_finish(e, job))) {
    e->fs.gradient_ran_on_garbage();
    if (factorize_retry_after_abort(e, rc) != GMB_OK) return rc;
    rc_grad = grad ? grad_accumulate(e, h, nullptr) : GMB_OK;  // (an abandoned tile launch: the recursion's factor, the gradient again)
  }
  if (rc_grad) return rc_grad;
  *nlml = 0.5 * (double)e->N * std::log(2.0 * M_PI) + e->logdet + 0.5 * e->vnorm2;
  return grad ? grad_chain_rule(e, h, grad) : GMB_OK;
}

}  // extern "C"

namespace {

// ---- the split-k product (gemm_splitk.hpp) and the bordered update of the resident factor (gmb_append / gmb_truncate) ------------

// C = beta C + alpha A B^T on few tiles with a long contraction: the launch pair, partials in the engine's workspace.  `pin` >= 1
// fixes the number of slices (refused when a slice would be empty), anything else leaves it to splitk_rule; *used = what ran.
int launch_gemm_splitk(gmb_engine* e, hipStream_t s, SplitKArgs a, int pin, int32_t* used) {
  if (used) *used = 0;
  if (a.mt <= 0 || a.nt <= 0 || a.k <= 0) return GMB_OK;
  const int tiles = splitk_tile_count(a.mt, a.nt, a.tri);
  if (tiles <= 0) return GMB_OK;
  if (tiles > 65535) return fail(e, GMB_EINVAL, "split-k GEMM: %d output tiles (at most 65535: it is the kernel for FEW tiles)", tiles);
  int len = 0, S = pin;
  if (pin >= 1) {
    len = splitk_pinned_len(a.k, pin);
    if (!len) return fail(e, GMB_EINVAL, "split-k GEMM: %d slices of k = %d leave a slice empty", pin, a.k);
  } else {
    S = splitk_rule(tiles, a.k, &len);
  }
  int rc;
  if ((rc = e->dsk.reserve(e->pool, (int64_t)tiles * S * TILE * TILE))) return rc;
  a.slices = S;
  a.slice_len = len;
  a.ws = e->dsk;
  ev_begin(e, s, EV_SPLITK, 2.0 * TILE * TILE * (double)a.k * tiles, a.mt, a.nt, a.k, S);
  hipLaunchKernelGGL(gemm_f64_splitk_partial_kernel, dim3((unsigned)S, (unsigned)tiles), dim3(256), 0, s, a);
  hipLaunchKernelGGL(gemm_f64_splitk_reduce_kernel, dim3(TILE * TILE / 256, (unsigned)tiles), dim3(256), 0, s, a);
  ev_end(e);
  HIP_TRY(e, hipGetLastError());
  if (used) *used = S;
  return GMB_OK;
}

// a complete, unconsumed single-engine factor of the current (data, kernel, theta) sits in dA
bool has_live_factor(const gmb_engine* e) {
  return e->fs.live_single() && e->dA && e->dA.cap > 0;
}

// what gmb_append and gmb_truncate refuse alike
int resize_ready(gmb_engine* e, const char* what) {
  int rc = require_ready(e, false);
  if (rc) return rc;
  if (e->solve_hook || e->dist_mode != 0 || e->fs.distributed())
    return fail(e, GMB_EINVAL, "%s is not available on distributed engines (gmb_dist_*, capacity mode)", what);
  if (e->fs.valid_but_consumed())
    return fail(e, GMB_EINVAL, "%s: the factor was consumed by a gradient call: call gmb_factorize again", what);
  return GMB_OK;
}

// Block rows >= I0 of the bordered factor from scratch, against the block columns [0, I0) the buffer still holds: covariance
// rows, panel solve, corner update (split-k), Cholesky of the corner, log-det, v -- and the host's look (factorize_finish).
// The engine's sizes, points and buffers are the NEW ones already.  I0 = 0 is a whole factorisation by this route.
int refactor_tail(gmb_engine* e, const AppendLayout& lay) {
  int rc;
  const AppendRegions reg = append_regions(lay);
  const int I0 = (int)lay.I0, nct = (int)reg.nct, nrt = (int)reg.nrt;
  hipStream_t s = e->stream;
  begin_factorisation(e, FactorState::SINGLE, true);
  e->chol = CholResult{};
  FactorJob job;  // (the plain plan)
  // phase events as behind gmb_factorize: kbuild_ms = the rebuilt rows of Sigma, chol_ms = panel solve + corner update + corner
  // factorisation + v (tools/gpu_append.py)
  if ((rc = ensure_phase_events(e))) return rc;
  job.events_recorded = true;
  HIP_TRY(e, hipMemsetAsync(e->dscal, 0, (size_t)SCAL_GACC_AT * sizeof(double), s));
  const FactorRef f = train_factor(e);
  HIP_TRY(e, hipEventRecord(e->fe[0], s));
  {  // block rows >= I0 of Sigma: partial block row, new rows, y row, identity padding
    CovTileArgs a = train_cov_args(e, e->dA, e->ld, nrt, nct);
    a.row_first = I0;
    a.row_stride = 1;
    if ((rc = launch_train_cov(e, a))) return rc;
  }
  HIP_TRY(e, hipEventRecord(e->fe[1], s));
  HIP_TRY(e, hipEventRecord(e->fe[2], s));
  if (I0 > 0) {
    // P = Sigma[rows >= I0, :I0] L^-T in place in the factor buffer (the y row rides along: its part of v)
    if ((rc = trsm_cols(e, s, f, e->dA + reg.panel_off, e->ld, (int)reg.panel_row_tiles, 0, I0, EV_CHOL_SOLVE_GEMM, EV_CHOL_STRIP))) return rc;
    // corner -= P P^T: a handful of tiles contracted over every kept column
    SplitKArgs k{};
    k.C = e->dA + reg.corner_off;
    k.ldc = e->ld;
    k.A = k.B = e->dA + reg.panel_off;
    k.lda = k.ldb = e->ld;
    k.mt = (int)reg.corner_mt;
    k.nt = (int)reg.corner_nt;
    k.k = (int)reg.corner_k;
    k.alpha = -1.0;
    k.beta = 1.0;
    k.tri = 1;
    // ... when the corner IS a handful of tiles, or the rule finds slices to cut; a corner of many tiles (a large K) is the shape
    // launch_gemm's triangular update is built for: one workgroup per tile fills the chip, no workspace, C touched once
    const int corner_tiles = splitk_tile_count(k.mt, k.nt, 1);
    if (corner_tiles <= SPLITK_FEW_TILES || splitk_rule(corner_tiles, k.k, nullptr) > 1) {
      if ((rc = launch_gemm_splitk(e, s, k, -1, nullptr))) return rc;
    } else {
      GemmArgs g{};
      g.C = k.C;
      g.ldc = k.ldc;
      g.A = k.A;
      g.lda = k.lda;
      g.B = k.B;
      g.ldb = k.ldb;
      g.mt = k.mt;
      g.nt = k.nt;
      g.k = k.k;
      g.alpha = -1.0;
      g.beta = 1.0;
      g.tri = 1;
      if ((rc = launch_gemm(e, s, g, EV_CHOL_UPDATE))) return rc;
    }
    // the kept columns' share of the log-determinant; the corner's leaves add theirs
    hipLaunchKernelGGL(diag_logdet_kernel, dim3(1), dim3(256), 0, s, e->dA, e->ld, (int64_t)I0 * TILE, e->dscal);
    HIP_TRY(e, hipGetLastError());
  }
  // the corner by the plain recursion (launches only: it is a few block columns wide)
  if (I0 < nct && (rc = chol_cols(e, s, f, I0, nct, nrt, EV_CHOL_PANEL_GEMM))) return rc;
  hipLaunchKernelGGL(extract_v_kernel, dim3(EXTRACT_V_BLOCKS), dim3(TILE), 0, s, e->dA, e->ld, e->N, e->dv, e->dscal + 1);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->fe[3], s));
  if ((rc = ensure_host_landing(e))) return rc;
  HIP_TRY(e, hipMemcpyAsync(e->hl->scal, e->dscal, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(&e->hl->info, e->dinfo, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  job.in_flight = true;
  return factorize_finish(e, job);
}

// N -> N_new under the engine: K rows appended (Xnew, ynew) or the tail cut (Xnew == nullptr).  Kernel, periods and theta stay.
// Without a live factor the result is what gmb_set_data on the new arrays + gmb_set_theta would leave; with one, the factor is
// re-laid when its leading dimension or its capacity asks for it, and updated by refactor_tail.
int resize_n(gmb_engine* e, int64_t N_new, const double* Xnew, int64_t K, int64_t ldx, const double* ynew, int32_t memspace,
             const char* what) {
  HIP_TRY(e, hipSetDevice(e->device));
  const bool live = has_live_factor(e);
  // sizes, kept block columns and copy plan: append_layout.hpp (host arithmetic that tools/append_layout_check.cpp runs under sanitizers)
  const AppendLayout lay = append_layout(e->N, e->ld, N_new, e->dA ? e->dA.cap : 0);
  const int64_t N_old = lay.N_old, Np_old = lay.Np_old, ld_old = lay.ld_old;
  const int64_t Np_new = lay.Np_new, Nr_new = lay.Nr_new, ld_new = lay.ld_new;
  const int I0 = (int)lay.I0;
  const int D = e->D;
  int rc;
  // the re-laid factor first: a device that cannot hold both copies refuses before anything is touched
  ScopedBuf<double> newA(e->pool);
  if (live && lay.relayout) {
    const double need = 8.0 * (double)ld_new * (double)Np_new;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(e, hipMemGetInfo(&free_b, &total_b));
    if (need > (double)free_b)
      return fail(e, GMB_ENOMEM, "%s: re-laying the factor for N = %lld (leading dimension %lld -> %lld) needs %.0f bytes beside the resident "
                                 "copy, %.0f are free -- nothing was changed", what, (long long)N_new, (long long)ld_old, (long long)ld_new, need, (double)free_b);
    if ((rc = newA.reserve(e->pool, ld_new * Np_new))) return rc;
  }
  e->fs.resized(live);
  e->fitc.resident = false;
  e->lap.drop("gmb_append / gmb_truncate changed the data");
  auto bail = [&](int code) {  // a failure half-way: no factor; the data may be of either size, so nothing is ready
    e->fs.resize_failed();
    e->have_theta = false;
    return code;
  };
  const hipMemcpyKind kind = memspace == GMB_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (Xnew) {  // append: new X and y buffers, the old rows in front
    ScopedBuf<double> nX(e->pool), ny(e->pool);
    if ((rc = nX.reserve(e->pool, N_new * (int64_t)D)) || (rc = ny.reserve(e->pool, Np_new))) return bail(rc);
    hipError_t hs = hipMemcpyAsync(nX, e->dX, (size_t)(N_old * D) * sizeof(double), hipMemcpyDeviceToDevice, e->stream);
    if (hs == hipSuccess) hs = hipMemcpy2DAsync(nX + N_old * D, D * sizeof(double), Xnew, ldx * sizeof(double), D * sizeof(double), K, kind, e->stream);
    if (hs == hipSuccess) hs = hipMemsetAsync(ny, 0, (size_t)Np_new * sizeof(double), e->stream);
    if (hs == hipSuccess) hs = hipMemcpyAsync(ny, e->dy, (size_t)N_old * sizeof(double), hipMemcpyDeviceToDevice, e->stream);
    if (hs == hipSuccess) hs = hipMemcpyAsync(ny + N_old, ynew, (size_t)K * sizeof(double), kind, e->stream);
    if (hs == hipSuccess) hs = hipStreamSynchronize(e->stream);  // the caller may reuse its buffers
    if (hs != hipSuccess) return bail(fail(e, GMB_EHIP, "%s: copying the new observations failed: %s", what, hipGetErrorString(hs)));
    e->dX.adopt(e->pool, nX);
    e->dy.adopt(e->pool, ny);
    if (Np_new > Np_old) {
      if ((rc = e->dv.renew(e->pool, Np_new))) return bail(rc);
      const int64_t need = (Np_new / TILE) * (int64_t)8 * 256;
      if (e->dDinv16.cap < need) {  // the kept blocks' sub-block inverses move along
        ScopedBuf<double> nd(e->pool);
        if ((rc = nd.reserve(e->pool, need))) return bail(rc);
        if (live && I0 > 0 && hipMemcpy(nd, e->dDinv16, (size_t)I0 * 8 * 256 * sizeof(double), hipMemcpyDeviceToDevice) != hipSuccess)
          return bail(fail(e, GMB_EHIP, "%s: copying the kept blocks' sub-block inverses failed", what));
        e->dDinv16.adopt(e->pool, nd);
      }
    }
  } else {  // truncate: the buffers stay, y's padding is zero again
    if (hipMemsetAsync(e->dy + N_new, 0, (size_t)(Np_old - N_new) * sizeof(double), e->stream) != hipSuccess)
      return bail(fail(e, GMB_EHIP, "%s: clearing the padding of y failed", what));
  }
  // sizes, and everything sized by them (as gmb_set_data drops it)
  e->N = N_new;
  e->Np = Np_new;
  e->Nr = Nr_new;
  e->ld = ld_new;
  stale_sized_by_n(e);
  // the prepared coordinates of ALL rows: their SoA stride is Nr
  if ((rc = e->pts.reserve(e->pool, e->Nr))) return bail(rc);
  if ((rc = prep_points(e, e->dX, e->N, e->D, e->Nr, e->pts.xs, e->pts.xl, e->pts.cat))) return bail(rc);
  if (!live) {
    if (hipStreamSynchronize(e->stream) != hipSuccess) return bail(fail(e, GMB_EHIP, "%s: preparing the points failed", what));
    if (e->dA.cap < e->ld * e->Np) e->dA.drop(e->pool);  // (gmb_set_data: a factor buffer too small for the new size goes)
    return GMB_OK;
  }
  if (newA) {  // the kept lower triangle, block column by block column: rows [128 c, 128 I0) of columns [128 c, 128 c + 128)
    for (int c = 0; c < I0; ++c) {
      const AppendCopy cp = append_copy_block(lay, c);
      const hipError_t hs = hipMemcpy2DAsync(newA + cp.dst, ld_new * sizeof(double), e->dA + cp.src, ld_old * sizeof(double),
                                             (size_t)cp.rows * sizeof(double), (size_t)cp.cols, hipMemcpyDeviceToDevice, e->stream);
      if (hs != hipSuccess) return bail(fail(e, GMB_EHIP, "%s: re-laying the factor failed: %s", what, hipGetErrorString(hs)));
    }
    if (hipStreamSynchronize(e->stream) != hipSuccess) return bail(fail(e, GMB_EHIP, "%s: re-laying the factor failed", what));
    e->dA.adopt(e->pool, newA);
  }
  return refactor_tail(e, lay);
}

// M is tiled so that the solved cross-covariance (Mt x Np doubles) stays within ~8 GiB
int64_t predict_tile_rows(const gmb_engine* e, int64_t M) {
  int64_t mt_max = (int64_t)(8.0 * 1024 * 1024 * 1024 / 8.0 / (double)e->Np);
  mt_max = std::max<int64_t>(TILE, std::min<int64_t>(mt_max / TILE * TILE, 32768));
  return std::min<int64_t>(round_up(M, TILE), mt_max);
}

// Every allocation of gmb_predict for M-tiles of Mt rows.  The capacity driver calls it BEFORE its ranks agree to start a
// prediction: a rank that ran out of memory here would otherwise leave gmb_predict before the solve hook, i.e. without
// issuing the pass's all-gathers, with its peers blocked inside them.
int predict_workspace(gmb_engine* e, int64_t Mt) {
  Reserver take{e->pool};
  predict_buffers(*e, (double)Mt, take);
  return take.rc;
}

// what a guarded call holds its Budget against: the bytes the device has free now
int device_free_bytes(gmb_engine* e, double* free_bytes) {
  size_t free_b = 0, total_b = 0;
  HIP_TRY(e, hipMemGetInfo(&free_b, &total_b));
  *free_bytes = (double)free_b;
  return GMB_OK;
}

// ---- the pieces of one M-tile of a prediction, shared by gmb_predict (tile by tile) and the joint posterior (all M rows at
// once, engine.hip: joint_covariance) ----------------------------------------------------------------------------------------

// Which form V = K(X*, X) L^-T takes (gmb_set_predict_form): the product with the resident inverse factor needs what the tile
// path's gradient leaves behind; everything else is the triangular solve.
bool predict_takes_gemm_form(const gmb_engine* e) {
  return !e->solve_hook && e->predict_form != 0 && e->fs.gemm_form_ready() && e->dW && e->dUdiag && e->dW.cap >= e->Np * e->Np;
}

// mc test points (Xs: their first row) -> prepared points in txs / txl / tcat, the cross-covariance K(X*, X) in dV (mpad x Np,
// test index fastest) and the prior variances (+ noise) in dkss
int predict_cross_cov(gmb_engine* e, uint32_t terms, const double* Xs, int64_t mc, int64_t mpad, int64_t ldxs, int32_t with_noise,
                      hipMemcpyKind in_kind) {
  int rc;
  HIP_TRY(e, hipMemcpy2DAsync(e->pw.dXs, e->D * sizeof(double), Xs, ldxs * sizeof(double),
                              e->D * sizeof(double), mc, in_kind, e->stream));
  const PointSet test{e->pw.txs, e->pw.txl, e->pw.tcat, mc, mpad};
  // the first selected term writes, an additive model's further terms add (the noise is the first pass's)
  const int t_first = first_term(terms);
  return walk_terms(e, terms, [&](int t) -> int {
    const gmb_engine::Term& tr = e->terms[t];
    const bool first = t == t_first;
    if ((rc = prep_points(e, e->pw.dXs, mc, e->D, mpad, e->pw.txs, e->pw.txl, e->pw.tcat, &tr.pa))) return rc;
    CovTileArgs a{};  // cross-covariance W[m + i*mpad] = k(x*_m, x_i)
    a.p = tr.cp;
    a.rows = test;
    a.cols = train_set(e);
    a.out = e->pw.dV;
    a.ldo = mpad;
    a.ti = (int)(mpad / TILE);
    a.tj = (int)(e->Np / TILE);
    a.mode = COV_CROSS;
    a.accumulate = !first;
    if (first) ev_begin(e, e->stream, EV_PREDICT_COV, 0.0, a.ti, a.tj);  // (while profiling: the launch on its own in GMB_TRACE_FILE)
    rc = launch_cov(e, a);
    if (first) ev_end(e);
    if (rc) return rc;
    KssArgs k{};
    k.p = first ? first_pass_params(e, t) : tr.cp;
    k.pts = test;
    k.with_noise = first ? with_noise : 0;
    k.accumulate = !first;
    k.kss = e->pw.dkss;
    hipLaunchKernelGGL(kss_kernel, dim3((unsigned)((mpad + 255) / 256)), dim3(256), 0, e->stream, k);
    return GMB_OK;
  });
}

// V <- V L^-T in dV (the solve), or V^T = L^-1 K(X, X*) into dV2 with the cross-covariance left in dV (`gemm_form`)
int predict_solve_v(gmb_engine* e, int64_t mpad, bool use_gemm_form) {
  int rc;
  // the triangular solve V <- V L^-T: one persistent launch for the matrices the tile Cholesky factors, else the recursion
  const int nblocks = (int)(e->Np / TILE);
  // (measured window, r03: faster than the recursion whenever the launch has enough tile tasks to fill the chip --
  // row tiles x block columns >= 576: 1000 test points at N = 10k 4.05 -> 3.25 ms, 2500 at N = 5k 2.15 -> 1.86, 640 at
  // N = 16k 6.55 -> 5.24, 384 at N = 28k 12.7 -> 8.9; 5 - 10 % for the standard 10^4-point grid -- and slower below
  // that (a few row tiles walk the block columns as a chain either way, the recursion's launches are lighter), and for
  // 4 x 10^4 points, where the recursion's large GEMMs run at 73 TF/s against the persistent loop's 69;
  // scheme 3 forces it for any size; tools/gpu_chol_tiles.py CT_PREDICT=1)
  const int ntm = (int)(mpad / TILE);
  const bool by_size = nblocks >= e->tiles_trsm_min_blocks && nblocks <= e->tiles_max_blocks &&
                       (ntm >= 32 || (long long)ntm * nblocks >= 576);
  const bool tiles = !e->naive_leaf && ntm <= 96 && (e->chol_scheme == 3 || (e->chol_scheme < 0 && by_size));
  bool tile_solve = false;  // the solve ran on the tile kernel, whose abort word is read back below
  if (e->solve_hook) {
    if ((rc = e->solve_hook(e->pw.dV, mpad, (int)(mpad / TILE)))) return rc;
  } else if (use_gemm_form) {
    // U = L^-T of this factor is resident (the fit's last evaluation left it): V^T = L^-1 K(X, X*) as ONE product with a
    // triangular operand (predict_form.hpp) instead of a solve
    if (e->fs.linv_missing()) {
      LinvArgs la{};
      la.U = e->dA;
      la.ldu = e->ld;
      la.udiag = e->dUdiag;
      la.W = e->dW;
      la.ldw = e->Np;
      la.nct = nblocks;
      hipLaunchKernelGGL(linv_from_u_kernel, dim3((unsigned)((long long)nblocks * (nblocks + 1) / 2)), dim3(256), 0, e->stream, la);
      HIP_TRY(e, hipGetLastError());
      e->fs.linv_transposed();
    }
    GemmArgs g{};
    g.C = e->pw2.dV2;
    g.ldc = e->Np;
    g.A = e->pw.dV;
    g.lda = mpad;
    g.B = e->dW;
    g.ldb = e->Np;
    g.mt = ntm;
    g.nt = nblocks;
    g.k = (int)e->Np;
    g.alpha = 1.0;
    g.beta = 0.0;
    g.khi_n = 1;
    if ((rc = launch_gemm(e, e->stream, g, EV_PREDICT_GEMM))) return rc;
  } else if ((rc = tiles ? trsm_tiles(e, e->stream, train_factor(e), e->pw.dV, mpad, ntm, EV_PREDICT_GEMM, &tile_solve)
                         : trsm_cols(e, e->stream, train_factor(e), e->pw.dV, mpad, ntm, 0, nblocks, EV_PREDICT_GEMM, EV_SOLVE_STRIP)))
    return rc;
  if (tile_solve) {  // a launch that gave up waiting must not be mistaken for a prediction
    uint32_t ab = 0;
    HIP_TRY(e, hipMemcpyAsync(&ab, e->dct + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    if (ab != 0) return fail(e, GMB_EHIP, "tile triangular solve: a workgroup waited longer than its time-out for a tile (launch abandoned)");
  }
  return GMB_OK;
}

// mean and variance of the tile's mc points into dmean / dvar
int predict_reduce(gmb_engine* e, int64_t mc, int64_t mpad, bool gemm_form) {
  const int nchunk = red_chunks(e->N);
  if (gemm_form) {
    // variance from Vt, mean = K(X*, X) alpha from the cross-covariance, which the GEMM left in dV (predict_form.hpp)
    hipLaunchKernelGGL(predict_rows_kernel, dim3((unsigned)mc), dim3(256), 0, e->stream, e->pw2.dV2, e->Np, e->N, e->pw.dkss, e->pw.dvar);
    hipLaunchKernelGGL(predict_mean_partial_kernel, dim3((unsigned)(mpad / 256 + (mpad % 256 ? 1 : 0)), nchunk),
                       dim3(256), 0, e->stream, e->pw.dV, mpad, e->dalpha, e->N, e->dpart, mpad);
    hipLaunchKernelGGL(predict_mean_final_kernel, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, e->stream, e->dpart, nchunk,
                       mpad, mc, e->pw.dmean);
    HIP_TRY(e, hipGetLastError());
  } else {
    double* pmu = e->dpart;
    double* ps = e->dpart + (int64_t)nchunk * mpad;
    hipLaunchKernelGGL(predict_partial_kernel, dim3((unsigned)(mpad / 256 + (mpad % 256 ? 1 : 0)), nchunk),
                       dim3(256), 0, e->stream, e->pw.dV, mpad, e->dv, e->N, pmu, ps, mpad);
    hipLaunchKernelGGL(predict_final_kernel, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, e->stream,
                       pmu, ps, nchunk, mpad, e->pw.dkss, mc, e->pw.dmean, e->pw.dvar);
    HIP_TRY(e, hipGetLastError());
  }
  return GMB_OK;
}

// ---- the joint posterior (joint_predict.hpp): full covariance and correlated draws ----------------------------------------------

// C as the Cholesky's routines take it (buffers and capacities stay JointState's)
FactorRef joint_factor_ref(JointState& jt) { return FactorRef{jt.dC, jt.Mr, jt.M, jt.Mp, jt.Mr, jt.dDinv16, jt.dscal, &jt.dct}; }

// what both calls ask of the engine: a complete single-engine factor on this device
int joint_ready(gmb_engine* e, const char* what) {
  int rc = require_ready(e, true);
  if (rc) return rc;
  if (e->solve_hook || e->dist_mode != 0 || !e->fs.single())
    return fail(e, GMB_EINVAL, "%s is not available on distributed engines (gmb_dist_*, capacity mode): factorise with gmb_factorize on one device", what);
  if ((rc = require_full_factor(e, what))) return rc;
  if (e->fs.consumed()) return fail(e, GMB_EINVAL, "the factor was consumed by a gradient call: call gmb_factorize again");
  return GMB_OK;
}

// What a joint posterior at M points (mr x mp in the bordered layout) gets AFTER its guard's check: the small fixed buffers of the
// factorisation of C -- sub-block inverses, scalar block, zero row -- are in no budget, O(M) beside the O(M N + M^2) measured.
int joint_fixed_buffers(gmb_engine* e, int64_t M, int64_t mr, int64_t mp) {
  JointState& jt = e->jt;
  int rc;
  if ((rc = jt.dDinv16.reserve(e->pool, (mp / TILE) * (int64_t)8 * 256))) return rc;
  if ((rc = jt.dscal.reserve(e->pool, (int64_t)SCAL_GACC_AT))) return rc;
  if (jt.dzero.cap < mr) {
    if ((rc = jt.dzero.reserve(e->pool, mr))) return rc;
    HIP_TRY(e, hipMemsetAsync(jt.dzero, 0, (size_t)jt.dzero.cap * sizeof(double), e->stream));
  }
  jt.M = M, jt.Mp = mp, jt.Mr = mr;
  return GMB_OK;
}

// Every buffer of a joint prediction at M points (+ `stage` doubles of device staging for host-side arguments), allocated
// before anything is launched.  V is held whole -- the rank-N update needs every pair of its row tiles -- so a request is
// first measured against the device: one that cannot fit is refused with the bytes it needs, and nothing has been touched.
// The buffers are joint_buffers' list (workspaces.hpp), walked by the budget and then by the allocation.
int joint_workspace(gmb_engine* e, const char* what, int64_t M, bool gemm_form, double stage) {
  const int64_t mr = round_up(M + 1, TILE), mp = round_up(M, TILE);
  const double Mr = (double)mr, Mp = (double)mp;
  Budget need;
  joint_buffers(*e, Mr, Mp, gemm_form, stage, need);
  double free_b;
  int rc;
  if ((rc = device_free_bytes(e, &free_b))) return rc;
  if (need.fresh > free_b || Mr > 1073741824.0)  // (V's bytes: what the product form's second V takes)
    return fail(e, GMB_ENOMEM, "%s: M = %lld behind N = %lld needs %.0f bytes on the device (V: %.0f%s, C: %.0f), %.0f more than it holds "
                               "for the engine now; %.0f bytes are free -- nothing was computed",
                what, (long long)M, (long long)e->N, need.total, e->pw2.bytes(Mr, e->Np), gemm_form ? " twice" : "",
                sizeof(double) * joint_matrix_elems(Mr, Mp), need.fresh, free_b);
  Reserver take{e->pool};
  joint_buffers(*e, Mr, Mp, gemm_form, stage, take);
  return take.rc ? take.rc : joint_fixed_buffers(e, M, mr, mp);
}

// The posterior mean of all M points into dmean and the lower-triangle tiles of
//   C = K(X*, X*) - V V^T (+ noise) + jitter I
// into jt.dC (bordered layout of the training build: Mr x Mp, identity on the padding, a zero row where y would sit).
int joint_covariance(gmb_engine* e, uint32_t terms, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise, double jitter,
                     bool gemm_form, hipMemcpyKind in_kind) {
  JointState& jt = e->jt;
  const int64_t Mr = jt.Mr, Mp = jt.Mp;
  int rc;
  // V for all M points at once, in the form gmb_predict would take, and the mean by gmb_predict's own reductions
  if ((rc = predict_cross_cov(e, terms, Xs, M, Mr, ldxs, with_noise, in_kind))) return rc;
  if ((rc = predict_solve_v(e, Mr, gemm_form))) return rc;
  if ((rc = predict_reduce(e, M, Mr, gemm_form))) return rc;
  // the product form leaves V with the training index fastest: turned into the update's k-major layout (the cross-covariance
  // in dV has served the mean)
  if (gemm_form && (rc = launch_transpose(e, e->stream, e->pw2.dV2, e->Np, e->pw.dV, Mr, (int)e->Np, (int)Mr))) return rc;
  // Columns N .. Np-1 of V belong to no training point.  gmb_predict never reads them (its reductions stop at N); the update
  // below contracts over all Np, so they are cleared, whichever form produced them.
  if (e->Np > e->N)
    HIP_TRY(e, hipMemsetAsync(e->pw.dV + e->N * Mr, 0, (size_t)((e->Np - e->N) * Mr) * sizeof(double), e->stream));

  // K(X*, X*): the training build's launch (build_sigma) on the test points -- direct distances on the diagonal tiles, so the
  // diagonal is gmb_predict's k** to the bit.  Both point sets are the TEST points (workspace): the terms are visited without
  // walk_terms, nothing resident is re-prepared.  predict_cross_cov left the test points with the last selected term's
  // preparation, so a selection of one term builds on it as it is.  The first selected term's pass stores -- identity padding,
  // zero border row, and the model's noise and the call's jitter on the diagonal (first_pass_params) -- and the others add.
  const int nterms = (int)e->terms.size();
  int nsel = 0;
  for (int t = 0; t < nterms; ++t) nsel += (int)((terms >> t) & 1u);
  const PointSet test{e->pw.txs, e->pw.txl, e->pw.tcat, M, Mr};
  CovTileArgs a{};
  a.rows = test;
  a.cols = test;
  a.out = jt.dC;
  a.ldo = Mr;
  a.ti = (int)(Mr / TILE);
  a.tj = (int)(Mp / TILE);
  a.mode = COV_TRAIN;
  a.lower_only = 1;
  a.tri_grid = 1;
  a.y = jt.dzero;
  bool first = true;
  for (int t = 0; t < nterms; ++t) {
    if (!((terms >> t) & 1u)) continue;
    if (nsel > 1 && (rc = prep_points(e, e->pw.dXs, M, e->D, Mr, e->pw.txs, e->pw.txl, e->pw.tcat, &e->terms[t].pa))) return rc;
    if (first) {
      a.p = first_pass_params(e, t);
      if (!with_noise) a.p.sigma2 = 0.0;
      a.p.jitter = jitter;
    } else {
      a.p = e->terms[t].cp;
      a.accumulate = 1;
    }
    if ((rc = launch_cov(e, a))) return rc;
    first = false;
  }

  // C -= V V^T: the trailing update's launch with contraction length Np (rows of the border stay as built: V is zero there)
  GemmArgs g{};
  g.C = jt.dC;
  g.ldc = Mr;
  g.A = e->pw.dV;
  g.lda = Mr;
  g.B = e->pw.dV;
  g.ldb = Mr;
  g.mt = (int)(Mp / TILE);
  g.nt = (int)(Mr / TILE);
  g.k = (int)e->Np;
  g.alpha = -1.0;
  g.beta = 1.0;
  g.tri = 1;
  return launch_gemm(e, e->stream, g, EV_PREDICT_GEMM);
}

// C -> L* in place, by the schedule gmb_factorize would give a matrix of this size (chol_factor: the persistent tile kernel from
// six block columns on, the recursion with tile-kernel panels otherwise; never the masked look-ahead, untraced, no injected
// faults).  The factorisation is told its matrix, so nothing of the training factorisation is read or written.  Synchronises;
// an abandoned tile launch is an error.
int joint_factor(gmb_engine* e) {
  JointState& jt = e->jt;
  HIP_TRY(e, hipMemsetAsync(jt.dscal, 0, (size_t)SCAL_GACC_AT * sizeof(double), e->stream));
  const FactorRef f = joint_factor_ref(jt);
  CholResult res;
  int rc = chol_factor(e, f, CholOpts{}, &res);
  if (rc) return rc;
  int32_t info = 0;
  uint32_t ab = 0;
  HIP_TRY(e, hipMemcpyAsync(&info, f.info(), sizeof info, hipMemcpyDeviceToHost, e->stream));
  if (res.tiles) HIP_TRY(e, hipMemcpyAsync(&ab, jt.dct + 1, sizeof ab, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  if (ab != 0)
    return fail(e, GMB_EHIP, "joint posterior: the tile Cholesky of the predictive covariance waited longer than its time-out for a tile (launch abandoned)");
  if (info != 0) {
    e->notpd = (int64_t)info - 1;
    return fail(e, GMB_ENOTPD, "the posterior covariance of the test points is not positive definite at row %lld (raise the jitter)",
                (long long)e->notpd);
  }
  return GMB_OK;
}

int launch_draw(gmb_engine* e, const DrawArgs& a) {
  const unsigned nrb = (unsigned)((a.M + 15) / 16);
  if (a.S <= 16) hipLaunchKernelGGL(joint_draw_kernel<1>, dim3(nrb, 1), dim3(256), 0, e->stream, a);
  else if (a.S <= 32) hipLaunchKernelGGL(joint_draw_kernel<2>, dim3(nrb, 1), dim3(256), 0, e->stream, a);
  else hipLaunchKernelGGL(joint_draw_kernel<4>, dim3(nrb, (unsigned)((a.S + 63) / 64)), dim3(256), 0, e->stream, a);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// ---- gradients of the posterior mean and variance (predict_grad.hpp) -----------------------------------------------------------------

// one term's partials, `nset` accumulator sets, for the prepared test points in pg_xs / pg_xl / pg_cat
int launch_predict_grad(gmb_engine* e, const PredGradArgs& a, int nchunk, int nset) {
  const dim3 grid((unsigned)(a.test.npad / PG_PTS), (unsigned)nchunk);
  const bool gen = a.p.n_lin > 0 || a.p.n_tab > 0;
  const bool known = with_kind_nc(a.p.kind, e->nc_pad, [&](auto kind, auto nc) {
    constexpr int K = decltype(kind)::value, NC = decltype(nc)::value;
    auto go = [&](void (*kernel)(PredGradArgs)) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, e->stream, a); };
    if (nset == 2) go(gen ? predict_grad_partial_kernel<K, NC, true, 2> : predict_grad_partial_kernel<K, NC, false, 2>);
    else go(gen ? predict_grad_partial_kernel<K, NC, true, 1> : predict_grad_partial_kernel<K, NC, false, 1>);
  });
  if (!known) return fail(e, GMB_EINVAL, "unknown kernel kind %d", a.p.kind);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// alpha = L^-T v into dalpha_bs by blocked back substitution against the resident factor (lower triangle of dA, diagonal tiles
// in place: the state every caller has checked -- complete single-engine factor, not consumed)
int backsub_alpha(gmb_engine* e) {
  int rc;
  if ((rc = e->dalpha_bs.reserve(e->pool, 2 * e->Np))) return rc;
  double* alpha = e->dalpha_bs;
  double* w = e->dalpha_bs + e->Np;
  const TriOperand L{e->dA, e->ld, e->dA, e->ld, (int64_t)TILE * (e->ld + 1)};
  const int nb = (int)(e->Np / TILE);
  ev_begin(e, e->stream, EV_PREDICT_GRAD_ALPHA, (double)e->N * (double)e->N, nb);
  HIP_TRY(e, hipMemcpyAsync(w, e->dv, e->N * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  for (int b = nb - 1; b >= 0; --b) {
    hipLaunchKernelGGL(backsub_diag_kernel, dim3(1), dim3(256), 0, e->stream, L, (int64_t)b, e->N, w, alpha);
    if (b > 0) hipLaunchKernelGGL(backsub_update_kernel, dim3((unsigned)(32 * b)), dim3(256), 0, e->stream, L, (int64_t)b, e->N, alpha, w);
  }
  ev_end(e);
  HIP_TRY(e, hipGetLastError());
  e->fs.back_substituted();
  return GMB_OK;
}

// W <- V L^-1 in dV (mpad rows, test index fastest) against the resident factor: block columns from the last
int predict_solve_w(gmb_engine* e, int64_t mpad) {
  const TriOperand L{e->dA, e->ld, e->dA, e->ld, (int64_t)TILE * (e->ld + 1)};
  const int nb = (int)(e->Np / TILE);
  ev_begin(e, e->stream, EV_PREDICT_VGRAD_SOLVE, (double)mpad * (double)e->N * (double)e->N, (int)(mpad / TILE), nb);
  for (int b = nb - 1; b >= 0; --b) {
    hipLaunchKernelGGL(vsolve_diag_kernel, dim3((unsigned)(mpad / VS_ROWS)), dim3(VS_ROWS), 0, e->stream, L, (int64_t)b, e->N, e->pw.dV, mpad);
    if (b > 0)
      hipLaunchKernelGGL(vsolve_update_kernel, dim3((unsigned)(mpad / VS_PTS), (unsigned)b), dim3(256), 0, e->stream, L, (int64_t)b, e->N,
                         e->pw.dV, mpad);
  }
  ev_end(e);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// the fit's alpha if one is resident (the gradient evaluation's, refined against L), else by back substitution, once per
// factorisation
int resident_alpha(gmb_engine* e, const double** alpha) {
  int rc;
  if (e->fs.needs_backsub() && (rc = backsub_alpha(e))) return rc;
  *alpha = e->fs.gradient_alpha() ? e->dalpha : e->dalpha_bs;
  return GMB_OK;
}

// workspaces of the gradient calls for M-tiles of Mt rows (a multiple of 128), beside a prediction's: nset = 1 for
// gmb_predict_grad, 2 for gmb_predict_with_grad
int predict_grad_workspace(gmb_engine* e, int64_t Mt, int nset) {
  int rc;
  if ((rc = e->pg.reserve(e->pool, Mt, e->D))) return rc;
  if (nset == 2 && (rc = e->vg_grad.reserve(e->pool, Mt * (int64_t)e->D))) return rc;
  // every M-tile of mpad <= Mt rows runs nchunk <= PG_TARGET_WGS / (mpad / 64) + 1 chunks (predict_grad_chunk), so its partials
  // -- nchunk x nset x (nc_pad + n_lin) x mpad doubles -- fit in this whatever its size
  const int64_t need = nset * ((int64_t)PG_TARGET_WGS * PG_PTS + Mt) * (e->nc_pad + MAX_LIN);
  return e->pg_part.reserve(e->pool, need);
}

// d mu / d x* of one M-tile (mc raw points on the device, D per row, first row Xs) into pg_grad (mc x D, row-major); with
// W = K(X*, X) Sigma^-1 of the tile (mpad rows, test index fastest) also d sigma^2 / d x* into vg_grad.  W == nullptr: the mean only.
int predict_grad_tile(gmb_engine* e, uint32_t terms, const double* Xs, int64_t mc, int64_t mpad, const double* alpha, const double* W) {
  int rc;
  const int nset = W ? 2 : 1;
  HIP_TRY(e, hipMemsetAsync(e->pg.grad, 0, (size_t)(mc * e->D) * sizeof(double), e->stream));
  if (W) HIP_TRY(e, hipMemsetAsync(e->vg_grad, 0, (size_t)(mc * e->D) * sizeof(double), e->stream));
  int64_t chunk;
  int nchunk;
  predict_grad_chunk(e->N, mpad, &chunk, &nchunk);
  const PointSet test{e->pg.xs, e->pg.xl, e->pg.cat, mc, mpad};
  return walk_terms(e, terms, [&](int t) -> int {
    const gmb_engine::Term& tr = e->terms[t];
    if ((rc = prep_points(e, Xs, mc, e->D, mpad, e->pg.xs, e->pg.xl, e->pg.cat, &tr.pa))) return rc;
    PredGradArgs a{};
    a.p = tr.cp;
    a.test = test;
    a.train = train_set(e);
    a.alpha = alpha;
    a.W = W;
    a.part = e->pg_part;
    a.chunk = chunk;
    ev_begin(e, e->stream, W ? EV_PREDICT_VGRAD : EV_PREDICT_GRAD, 0.0, (int)(mpad / PG_PTS), nchunk);
    rc = launch_predict_grad(e, a, nchunk, nset);
    if (!rc) {
      PredGradFinishArgs f{};
      f.part = e->pg_part;
      f.nchunk = nchunk;
      f.nc = tr.pa.nc;
      f.nc_pad = e->nc_pad;
      f.n_lin = tr.cp.n_lin;
      f.periodic = tr.pa.periodic;
      f.D = e->D;
      f.nset = nset;
      f.mpad = mpad;
      f.mc = mc;
      f.txs = e->pg.xs;
      for (int k = 0; k < tr.pa.nc; ++k) f.idx_cont[k] = tr.pa.idx_cont[k];
      if (tr.pa.periodic) {
        for (int d = 0; 2 * d < tr.pa.nc; ++d) f.scale[d] = 2.0 * M_PI * tr.pa.two_over_T[d];  // 2 * (2 pi / T_d)
      } else {
        for (int k = 0; k < tr.pa.nc; ++k) f.scale[k] = 2.0 * tr.pa.inv_ls[k];
      }
      for (int l = 0; l < tr.cp.n_lin; ++l) f.idx_lin[l] = tr.pa.idx_lin[l];
      f.tau = tr.cp.tau;
      f.grad = e->pg.grad;
      if (W) {
        f.dvar = e->vg_grad;
        f.n_tab = tr.cp.n_tab;
        for (int i = 0; i < MAX_TABS; ++i) f.tab_levels[i] = tr.cp.tab_levels[i], f.tab_off[i] = tr.cp.tab_off[i];
        f.tabs = tr.cp.tabs;
        f.txl = e->pg.xl;
        f.tcat = e->pg.cat;
      }
      hipLaunchKernelGGL(predict_grad_finish_kernel, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, e->stream, f);
    }
    ev_end(e);
    if (rc) return rc;
    HIP_TRY(e, hipGetLastError());
    return GMB_OK;
  });
}

// ---- what the five prediction entry points share -------------------------------------------------------------------------------

void reset_predict_timings(gmb_engine* e) {
  gmb_timings& tm = e->tm;
  tm.predict_ms = tm.predict_gemm_ms = tm.predict_gemm_flops = 0.0;
  tm.predict_gemm_launches = 0;
}

// how the caller's arrays are copied in and out
struct CopyKinds {
  hipMemcpyKind in, out;
};
CopyKinds copy_kinds(int32_t memspace) {
  if (memspace == GMB_DEVICE) return {hipMemcpyDeviceToDevice, hipMemcpyDeviceToDevice};
  return {hipMemcpyHostToDevice, hipMemcpyDeviceToHost};
}

// The ending of a prediction call, on every exit after its first launch (rc: what the call's work returned; tp: its phase
// timer, if it keeps one).  Whatever happened, the stream is drained and the launches' events are collected -- none stays
// behind for the next call's sums; predict_ms is set only by a call that succeeded; the call's own error goes before the
// synchronise's.
int predict_end(gmb_engine* e, PhaseTimer* tp, int rc) {
  if (tp) tp->stop();
  const hipError_t sync = hipStreamSynchronize(e->stream);
  if (tp && !rc && sync == hipSuccess) e->tm.predict_ms = tp->ms();
  ev_collect(e);
  if (rc) return rc;
  HIP_TRY(e, sync);
  return GMB_OK;
}

// The selection of a prediction call: `sel` null = every term (the entry points without a selection), else the caller's mask,
// refused -- before anything is launched -- when it is empty or names a term the model does not have.
int resolve_terms(gmb_engine* e, const uint32_t* sel, const char* what, uint32_t* mask) {
  const uint32_t all = all_terms_mask(e);
  if (!sel) {
    *mask = all;
    return GMB_OK;
  }
  if (*sel == 0 || (*sel & ~all))
    return fail(e, GMB_EINVAL, "%s: terms = 0x%x selects %s (the model has %d term%s: bits 0 .. %d)", what, (unsigned)*sel,
                *sel == 0 ? "nothing" : "a term the model does not have", (int)e->terms.size(), e->terms.size() == 1 ? "" : "s",
                (int)e->terms.size() - 1);
  *mask = *sel;
  return GMB_OK;
}

// the M-tile of gmb_predict_decompose: T stacked blocks within the prediction's 8 GiB rule
int64_t decompose_tile_rows(const gmb_engine* e, int64_t M) {
  const int64_t T = (int64_t)e->terms.size();
  const int64_t mt_max = predict_tile_rows(e, (int64_t)1 << 40);  // a prediction's largest M-tile behind this N
  return std::min<int64_t>(std::max<int64_t>(TILE, mt_max / T / TILE * TILE), round_up(M, TILE));
}

template <int NT>
void launch_term_gram_nt(gmb_engine* e, dim3 grid, int64_t ldz, int64_t mpad) {
  hipLaunchKernelGGL(term_gram_partial_kernel<NT>, grid, dim3(256), 0, e->stream, e->pw.dV, ldz, mpad, e->dv, e->N, e->tg.part);
}

// one M-tile of gmb_predict_decompose: the T cross-covariances stacked in dV, one solve, the reductions; results in tg.out
int decompose_tile(gmb_engine* e, const double* Xs, int64_t mc, int64_t mpad, int64_t ldxs, hipMemcpyKind in_kind) {
  int rc;
  const int T = (int)e->terms.size();
  const int64_t ldz = (int64_t)T * mpad;
  double* means = e->tg.out;
  double* cov = means + (int64_t)T * mpad;
  double* noise = cov + (int64_t)(T * (T + 1) / 2) * mpad;
  HIP_TRY(e, hipMemcpy2DAsync(e->pw.dXs, e->D * sizeof(double), Xs, ldxs * sizeof(double), e->D * sizeof(double), mc, in_kind, e->stream));
  const PointSet test{e->pw.txs, e->pw.txl, e->pw.tcat, mc, mpad};
  rc = walk_terms(e, all_terms_mask(e), [&](int t) -> int {
    const gmb_engine::Term& tr = e->terms[t];
    int r;
    if ((r = prep_points(e, e->pw.dXs, mc, e->D, mpad, e->pw.txs, e->pw.txl, e->pw.tcat, &tr.pa))) return r;
    CovTileArgs a{};  // term t's block: W[t mpad + m + i ldz] = k_t(x*_m, x_i)
    a.p = tr.cp;
    a.rows = test;
    a.cols = train_set(e);
    a.out = e->pw.dV + (int64_t)t * mpad;
    a.ldo = ldz;
    a.ti = (int)(mpad / TILE);
    a.tj = (int)(e->Np / TILE);
    a.mode = COV_CROSS;
    a.accumulate = 0;
    if ((r = launch_cov(e, a))) return r;
    KssArgs k{};
    k.p = tr.cp;
    k.pts = test;
    k.with_noise = 0;
    k.accumulate = 0;
    k.kss = e->pw.dkss + (int64_t)t * mpad;
    hipLaunchKernelGGL(kss_kernel, dim3((unsigned)((mpad + 255) / 256)), dim3(256), 0, e->stream, k);
    if (t == 0)  // (the test points hold term 0's preparation here)
      hipLaunchKernelGGL(term_noise_kernel, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, e->stream, tr.cp, test, noise);
    HIP_TRY(e, hipGetLastError());
    return GMB_OK;
  });
  if (rc) return rc;
  if ((rc = predict_solve_v(e, ldz, false))) return rc;  // all T blocks at once; neither dW nor U is touched
  const int nchunk = red_chunks(e->N);
  const dim3 grid((unsigned)((mpad + 255) / 256), (unsigned)nchunk);
  ev_begin(e, e->stream, EV_TERM_GRAM, 0.0, (int)(mpad / TILE), nchunk, T);
  switch (T) {
    case 1: launch_term_gram_nt<1>(e, grid, ldz, mpad); break;
    case 2: launch_term_gram_nt<2>(e, grid, ldz, mpad); break;
    case 3: launch_term_gram_nt<3>(e, grid, ldz, mpad); break;
    case 4: launch_term_gram_nt<4>(e, grid, ldz, mpad); break;
    case 5: launch_term_gram_nt<5>(e, grid, ldz, mpad); break;
    default: break;  // (gmb_predict_decompose has refused more than TG_MAX_TERMS terms)
  }
  hipLaunchKernelGGL(term_gram_final_kernel, dim3((unsigned)((mc + 255) / 256), (unsigned)tg_entries(T)), dim3(256), 0, e->stream,
                     e->tg.part, nchunk, T, mpad, e->pw.dkss, mc, means, cov);
  ev_end(e);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// ---- the posterior of the slope (predict_slope.hpp) ---------------------------------------------------------------------------------

// one term's derivative cross-covariance of an M-tile into the stacked dV (kinds 0 - 2 only: the others have no kernel, and
// gmb_predict_slope has refused them)
int launch_slope_cov(gmb_engine* e, const SlopeCovArgs& a) {
  const dim3 grid((unsigned)(a.test.npad / SC_PTS), (unsigned)(e->Np / SC_PIECE));
  const bool gen = a.p.n_lin > 0 || a.p.n_tab > 0;
  if (a.p.kind == GMB_MATERN12 || a.p.kind == GMB_EXPONENTIAL)
    return fail(e, GMB_EINVAL, "kernel kind %d has no derivative process", a.p.kind);
  const bool known = with_kind_nc(a.p.kind, e->nc_pad, [&](auto kind, auto nc) {
    constexpr int K = decltype(kind)::value, NC = decltype(nc)::value;
    if constexpr (K <= 2) {
      if (gen) hipLaunchKernelGGL((slope_cross_cov_kernel<K, NC, true>), grid, dim3(256), 0, e->stream, a);
      else hipLaunchKernelGGL((slope_cross_cov_kernel<K, NC, false>), grid, dim3(256), 0, e->stream, a);
    }
  });
  if (!known) return fail(e, GMB_EINVAL, "unknown kernel kind %d", a.p.kind);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// the differentiable model columns of a selection (slope_plan.hpp): the selected terms' continuous and linear columns
int slope_columns(gmb_engine* e, uint32_t terms, const char* what, SlopeColumns* cols) {
  *cols = SlopeColumns{};
  for (int t = 0; t < (int)e->terms.size(); ++t) {
    if (!((terms >> t) & 1u)) continue;
    const PrepArgs& pa = e->terms[t].pa;
    for (int k = 0; k < pa.nc; k += pa.periodic ? 2 : 1)
      for (int j = 0; j < k; j += pa.periodic ? 2 : 1)
        if (pa.idx_cont[j] == pa.idx_cont[k])
          return fail(e, GMB_EINVAL, "%s: column %d of X is two continuous dimensions of the kernel", what, pa.idx_cont[k]);
    if (!slope_add_columns(*cols, pa.idx_cont, pa.nc) || !slope_add_columns(*cols, pa.idx_lin, pa.n_lin))
      return fail(e, GMB_EINVAL, "%s: more than %d differentiable columns", what, SLOPE_MAX_COLS);
  }
  return GMB_OK;
}

// one M-tile of gmb_predict_slope: the Dc derivative cross-covariances stacked in dV, one solve, the reductions; results in the
// slope workspace's mean / var / cov, in the caller's layout
int slope_tile(gmb_engine* e, uint32_t terms, const SlopeColumns& cols, const double* Xs, int64_t mc, int64_t mpad, int64_t ldxs,
               hipMemcpyKind in_kind, bool with_cov) {
  int rc;
  const int dc = cols.n;
  const SlopeLayout lay{mpad, dc};
  const int64_t ldz = lay.ldz();
  HIP_TRY(e, hipMemcpy2DAsync(e->pw.dXs, e->D * sizeof(double), Xs, ldxs * sizeof(double), e->D * sizeof(double), mc, in_kind, e->stream));
  const PointSet test{e->pw.txs, e->pw.txl, e->pw.tcat, mc, mpad};
  const int t_first = first_term(terms);
  rc = walk_terms(e, terms, [&](int t) -> int {
    const gmb_engine::Term& tr = e->terms[t];
    const PrepArgs& pa = tr.pa;
    const bool first = t == t_first;
    int r;
    if ((r = prep_points(e, e->pw.dXs, mc, e->D, mpad, e->pw.txs, e->pw.txl, e->pw.tcat, &pa))) return r;
    SlopeCovArgs a{};
    SlopePriorArgs pr{};
    a.p = pr.p = tr.cp;
    a.test = pr.test = test;
    a.train = train_set(e);
    a.out = e->pw.dV;
    a.ldz = ldz;
    a.accumulate = pr.accumulate = first ? 0 : 1;
    a.periodic = pa.periodic;
    a.nc = pa.nc;
    a.dc = pr.dc = dc;
    uint32_t covered = 0;
    if (pa.periodic) {
      for (int d = 0; 2 * d < pa.nc; ++d) {
        const int c = cols.slot_of(pa.idx_cont[2 * d]);
        const double w = M_PI * pa.two_over_T[d];  // 2 pi / T_d
        a.slot[d] = c;
        a.scale[d] = 2.0 * w;
        pr.jj[c] = pa.inv_ls[2 * d] * pa.inv_ls[2 * d] * w * w;
        covered |= 1u << c;
      }
    } else {
      for (int k = 0; k < pa.nc; ++k) {
        const int c = cols.slot_of(pa.idx_cont[k]);
        a.slot[k] = c;
        a.scale[k] = 2.0 * pa.inv_ls[k];
        pr.jj[c] = pa.inv_ls[k] * pa.inv_ls[k];
        covered |= 1u << c;
      }
    }
    for (int l = 0; l < tr.cp.n_lin; ++l) {
      const int c = cols.slot_of(pa.idx_lin[l]);
      a.slot_lin[l] = c;
      a.lin_over[l] = (covered >> c) & 1u;
      pr.tl[c] = tr.cp.tau;
    }
    for (int l = 0; l < tr.cp.n_lin; ++l) covered |= 1u << a.slot_lin[l];
    a.zero_slots = ~covered & ((1u << dc) - 1u);
    if (first) ev_begin(e, e->stream, EV_SLOPE_COV, 0.0, (int)(mpad / TILE), (int)(e->Np / TILE), dc);
    r = launch_slope_cov(e, a);
    if (first) ev_end(e);
    if (r) return r;
    pr.prior = e->slope.prior;
    hipLaunchKernelGGL(slope_prior_kernel, dim3((unsigned)((mpad + 255) / 256)), dim3(256), 0, e->stream, pr);
    HIP_TRY(e, hipGetLastError());
    return GMB_OK;
  });
  if (rc) return rc;
  if ((rc = predict_solve_v(e, ldz, false))) return rc;  // all Dc blocks at once; neither dW nor U is touched
  const int nchunk = red_chunks(e->N);
  const dim3 grid((unsigned)((mpad + 255) / 256), (unsigned)nchunk, (unsigned)slope_pair_blocks(dc, with_cov));
  if (with_cov)
    hipLaunchKernelGGL(slope_gram_partial_kernel<true>, grid, dim3(256), 0, e->stream, e->pw.dV, ldz, mpad, e->dv, e->N, dc, e->slope.part);
  else
    hipLaunchKernelGGL(slope_gram_partial_kernel<false>, grid, dim3(256), 0, e->stream, e->pw.dV, ldz, mpad, e->dv, e->N, dc, e->slope.part);
  HIP_TRY(e, hipGetLastError());
  // the model's other columns (categories, the output index) have slope 0 and variance 0
  HIP_TRY(e, hipMemsetAsync(e->slope.mean, 0, (size_t)(mc * e->D) * sizeof(double), e->stream));
  HIP_TRY(e, hipMemsetAsync(e->slope.var, 0, (size_t)(mc * e->D) * sizeof(double), e->stream));
  if (with_cov) HIP_TRY(e, hipMemsetAsync(e->slope.cov, 0, (size_t)(mc * e->D * e->D) * sizeof(double), e->stream));
  SlopeFinishArgs f{};
  f.part = e->slope.part;
  f.prior = e->slope.prior;
  f.nchunk = nchunk;
  f.dc = dc;
  f.with_cov = with_cov ? 1 : 0;
  f.D = e->D;
  f.mpad = mpad;
  f.mc = mc;
  for (int c = 0; c < dc; ++c) f.col[c] = cols.col[c];
  f.mean = e->slope.mean;
  f.var = e->slope.var;
  f.cov = with_cov ? (double*)e->slope.cov : nullptr;
  hipLaunchKernelGGL(slope_finish_kernel, dim3((unsigned)((mc + 255) / 256), (unsigned)slope_entries(dc, with_cov)), dim3(256), 0, e->stream, f);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

int predict_slope_sel(gmb_engine* e, const uint32_t* sel, const char* what, const double* Xs, int64_t M, int64_t ldxs, double* dmean,
                      double* dvar, int64_t ldg, double* dcov, int64_t ldc, int32_t memspace) {
  int rc = joint_ready(e, what);
  if (rc) return rc;
  uint32_t terms;
  if ((rc = resolve_terms(e, sel, what, &terms))) return rc;
  if (M < 0 || (M > 0 && (!Xs || !dmean)) || ldxs < e->D || ldg < e->D) return fail(e, GMB_EINVAL, "bad Xs/M/ldxs/grad/ldg");
  if (dcov && ldc < (int64_t)e->D * e->D) return fail(e, GMB_EINVAL, "%s: ldc = %lld is less than D x D = %d", what, (long long)ldc, e->D * e->D);
  for (int t = 0; t < (int)e->terms.size(); ++t)
    if (((terms >> t) & 1u) && e->terms[t].cp.kind != GMB_EXPQUAD && e->terms[t].cp.kind != GMB_MATERN52 && e->terms[t].cp.kind != GMB_MATERN32)
      return fail(e, GMB_EINVAL, "%s: the process has no derivative: term %d is a %s kernel, which is not mean-square differentiable", what,
                  t, e->terms[t].cp.kind == GMB_MATERN12 ? "Matern-1/2" : "Exponential");
  SlopeColumns cols;
  if ((rc = slope_columns(e, terms, what, &cols))) return rc;
  if (M == 0) return GMB_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  reset_predict_timings(e);
  e->tm.predict_gemm_form = 0;  // the stacked V is always solved for, as in gmb_predict_decompose: neither dW nor U is touched
  const bool with_cov = dcov != nullptr;
  const int dc = cols.n;
  const int64_t Mt = std::min<int64_t>(slope_tile_rows(predict_tile_rows(e, (int64_t)1 << 40), dc), round_up(M, TILE));
  const int nchunk = red_chunks(e->N);
  // every allocation before the first launch: Dc stacked blocks in the prediction's workspace, the partials, the results
  if ((rc = predict_workspace(e, (int64_t)dc * Mt))) return rc;
  if ((rc = e->slope.reserve(e->pool, Mt, (int64_t)nchunk * slope_entries(dc, with_cov), e->D, with_cov))) return rc;
  const CopyKinds ck = copy_kinds(memspace);
  const size_t row = e->D * sizeof(double);
  PhaseTimer tp(e);
  auto tiles = [&]() -> int {
    for (int64_t m0 = 0; m0 < M; m0 += Mt) {
      const int64_t mc = std::min<int64_t>(Mt, M - m0);
      if ((rc = slope_tile(e, terms, cols, Xs + m0 * ldxs, mc, round_up(mc, TILE), ldxs, ck.in, with_cov))) return rc;
      if (hipMemcpy2DAsync(dmean + m0 * ldg, ldg * sizeof(double), e->slope.mean, row, row, mc, ck.out, e->stream) != hipSuccess ||
          (dvar && hipMemcpy2DAsync(dvar + m0 * ldg, ldg * sizeof(double), e->slope.var, row, row, mc, ck.out, e->stream) != hipSuccess) ||
          (dcov && hipMemcpy2DAsync(dcov + m0 * ldc, ldc * sizeof(double), e->slope.cov, row * e->D, row * e->D, mc, ck.out, e->stream) !=
                       hipSuccess))
        return fail(e, GMB_EHIP, "%s: copying the results out failed", what);
    }
    return GMB_OK;
  };
  return predict_end(e, &tp, tiles());
}

// ---- the selecting forms of the four prediction calls; `sel` null: every term, i.e. the calls without a selection ---------------

int predict_sel(gmb_engine* e, const uint32_t* sel, const char* what, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise,
                double* mean, double* var, int32_t memspace) {
  int rc = require_ready(e, true);
  if (rc) return rc;
  if (sel && (e->solve_hook || e->dist_mode != 0 || !e->fs.single()))
    return fail(e, GMB_EINVAL, "%s is not available on distributed engines (gmb_dist_*, capacity mode): factorise with gmb_factorize on one device", what);
  uint32_t terms;
  if ((rc = resolve_terms(e, sel, what, &terms))) return rc;
  if (M < 0 || (M > 0 && (!Xs || !mean || !var)) || ldxs < e->D)
    return fail(e, GMB_EINVAL, "bad Xs/M/ldxs/mean/var");
  if (M == 0) return GMB_OK;
  // (the capacity driver's passes come through here with their own triangular solve; everybody else reads the factor in dA)
  if ((rc = e->solve_hook ? require_capacity_factor(e, what) : require_full_factor(e, what))) return rc;
  if (e->fs.consumed())
    return fail(e, GMB_EINVAL, "the factor was consumed by a gradient call: call gmb_factorize again");
  HIP_TRY(e, hipSetDevice(e->device));
  reset_predict_timings(e);

  const int64_t Mt = predict_tile_rows(e, M);
  if ((rc = predict_workspace(e, Mt))) return rc;
  // the GEMM form needs the inverse factor the tile path's gradient leaves behind, and a second Mt x Np buffer
  const bool use_gemm_form = predict_takes_gemm_form(e);
  if (use_gemm_form && (rc = e->pw2.reserve(e->pool, Mt, e->Np))) return rc;
  e->tm.predict_gemm_form = use_gemm_form ? 1 : 0;

  const CopyKinds ck = copy_kinds(memspace);
  PhaseTimer tp(e);
  auto tiles = [&]() -> int {
    for (int64_t m0 = 0; m0 < M; m0 += Mt) {
      const int64_t mc = std::min<int64_t>(Mt, M - m0);
      const int64_t mpad = round_up(mc, TILE);
      if ((rc = predict_cross_cov(e, terms, Xs + m0 * ldxs, mc, mpad, ldxs, with_noise, ck.in))) return rc;
      if ((rc = predict_solve_v(e, mpad, use_gemm_form))) return rc;
      if ((rc = predict_reduce(e, mc, mpad, use_gemm_form))) return rc;
      HIP_TRY(e, hipMemcpyAsync(mean + m0, e->pw.dmean, mc * sizeof(double), ck.out, e->stream));
      HIP_TRY(e, hipMemcpyAsync(var + m0, e->pw.dvar, mc * sizeof(double), ck.out, e->stream));
    }
    return GMB_OK;
  };
  return predict_end(e, &tp, tiles());
}

int predict_grad_sel(gmb_engine* e, const uint32_t* sel, const char* what, const double* Xs, int64_t M, int64_t ldxs, double* grad,
                     int64_t ldg, int32_t memspace) {
  int rc = joint_ready(e, what);
  if (rc) return rc;
  uint32_t terms;
  if ((rc = resolve_terms(e, sel, what, &terms))) return rc;
  if (M < 0 || (M > 0 && (!Xs || !grad)) || ldxs < e->D || ldg < e->D) return fail(e, GMB_EINVAL, "bad Xs/M/ldxs/grad/ldg");
  if (M == 0) return GMB_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  // 16384 points per tile: 256 blocks of 64, i.e. four chunks of the training set -- partials of 4 x the tile's gradient
  const int64_t Mt = std::min<int64_t>(round_up(M, TILE), 16384);
  if ((rc = predict_grad_workspace(e, Mt, 1))) return rc;
  const double* alpha = nullptr;
  if ((rc = resident_alpha(e, &alpha))) return predict_end(e, nullptr, rc);
  const CopyKinds ck = copy_kinds(memspace);
  const size_t row = e->D * sizeof(double);
  auto tiles = [&]() -> int {
    for (int64_t m0 = 0; m0 < M; m0 += Mt) {
      const int64_t mc = std::min<int64_t>(Mt, M - m0);
      HIP_TRY(e, hipMemcpy2DAsync(e->pg.Xs, row, Xs + m0 * ldxs, ldxs * sizeof(double), row, mc, ck.in, e->stream));
      if ((rc = predict_grad_tile(e, terms, e->pg.Xs, mc, round_up(mc, TILE), alpha, nullptr))) return rc;
      if (hipMemcpy2DAsync(grad + m0 * ldg, ldg * sizeof(double), e->pg.grad, row, row, mc, ck.out, e->stream) != hipSuccess)
        return fail(e, GMB_EHIP, "%s: copying the gradient out failed", what);
    }
    return GMB_OK;
  };
  return predict_end(e, nullptr, tiles());
}

int predict_joint_sel(gmb_engine* e, const uint32_t* sel, const char* what, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise,
                      double jitter, double* mean, double* cov, int64_t ldc, int32_t memspace) {
  int rc = joint_ready(e, what);
  if (rc) return rc;
  uint32_t terms;
  if ((rc = resolve_terms(e, sel, what, &terms))) return rc;
  if (M < 0 || (M > 0 && (!Xs || !mean || !cov)) || ldxs < e->D || ldc < M || !(jitter >= 0.0))
    return fail(e, GMB_EINVAL, "bad Xs/M/ldxs/mean/cov/ldc/jitter");
  if (M == 0) return GMB_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const bool host = memspace != GMB_DEVICE;
  const bool gemm_form = predict_takes_gemm_form(e);
  if ((rc = joint_workspace(e, what, M, gemm_form, host ? (double)M * (double)M : 0.0))) return rc;
  reset_predict_timings(e);
  e->tm.predict_gemm_form = gemm_form ? 1 : 0;
  const CopyKinds ck = copy_kinds(memspace);
  PhaseTimer tp(e);
  auto work = [&]() -> int {
    if ((rc = joint_covariance(e, terms, Xs, M, ldxs, with_noise, jitter, gemm_form, ck.in))) return rc;
    SymArgs sa{};
    sa.C = e->jt.dC;
    sa.ldc = e->jt.Mr;
    sa.out = host ? e->jt.dstage : cov;
    sa.ldo = host ? M : ldc;
    sa.M = M;
    const unsigned nb = (unsigned)((M + 31) / 32);
    hipLaunchKernelGGL(joint_symmetrise_kernel, dim3(nb, nb), dim3(256), 0, e->stream, sa);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, hipMemcpyAsync(mean, e->pw.dmean, M * sizeof(double), ck.out, e->stream));
    if (host)
      HIP_TRY(e, hipMemcpy2DAsync(cov, ldc * sizeof(double), e->jt.dstage, M * sizeof(double), M * sizeof(double), M,
                                  hipMemcpyDeviceToHost, e->stream));
    return GMB_OK;
  };
  return predict_end(e, &tp, work());
}

int draw_joint_sel(gmb_engine* e, const uint32_t* sel, const char* what, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise,
                   double jitter, const double* Z, int64_t S, int64_t ldz, double* Y, int64_t ldy, double* mean, int32_t memspace) {
  int rc = joint_ready(e, what);
  if (rc) return rc;
  uint32_t terms;
  if ((rc = resolve_terms(e, sel, what, &terms))) return rc;
  if (M < 0 || S < 0 || S > 0x7fffffff || (M > 0 && S > 0 && (!Xs || !Z || !Y)) || ldxs < e->D || ldz < M || ldy < M || !(jitter >= 0.0))
    return fail(e, GMB_EINVAL, "bad Xs/M/ldxs/Z/S/ldz/Y/ldy/jitter");
  if (M == 0 || S == 0) return GMB_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const bool host = memspace != GMB_DEVICE;
  const bool gemm_form = predict_takes_gemm_form(e);
  if ((rc = joint_workspace(e, what, M, gemm_form, host ? 2.0 * (double)S * (double)M : 0.0))) return rc;
  reset_predict_timings(e);
  e->tm.predict_gemm_form = gemm_form ? 1 : 0;
  const CopyKinds ck = copy_kinds(memspace);
  PhaseTimer tp(e);
  auto work = [&]() -> int {
    if ((rc = joint_covariance(e, terms, Xs, M, ldxs, with_noise, jitter, gemm_form, ck.in))) return rc;
    if ((rc = joint_factor(e))) return rc;
    DrawArgs da{};
    da.L = e->jt.dC;
    da.ldl = e->jt.Mr;
    da.mean = e->pw.dmean;
    da.M = M;
    da.S = (int32_t)S;
    if (host) {
      double* dZ = e->jt.dstage;
      double* dY = e->jt.dstage + S * M;
      HIP_TRY(e, hipMemcpy2DAsync(dZ, M * sizeof(double), Z, ldz * sizeof(double), M * sizeof(double), S, hipMemcpyHostToDevice, e->stream));
      da.Z = dZ, da.ldz = M, da.Y = dY, da.ldy = M;
    } else {
      da.Z = Z, da.ldz = ldz, da.Y = Y, da.ldy = ldy;
    }
    if ((rc = launch_draw(e, da))) return rc;
    if (host)
      HIP_TRY(e, hipMemcpy2DAsync(Y, ldy * sizeof(double), da.Y, M * sizeof(double), M * sizeof(double), S, hipMemcpyDeviceToHost, e->stream));
    if (mean) HIP_TRY(e, hipMemcpyAsync(mean, e->pw.dmean, M * sizeof(double), ck.out, e->stream));
    return GMB_OK;
  };
  return predict_end(e, &tp, work());
}

// ---- leave-one-out and leave-group-out predictions of the training rows (leave_out.hpp) ---------------------------------------------

// what comes off 1 / d_i: the jitter, and the row's noise unless the caller wants it (noise, jitter and the output table are
// term 0's -- the preparation the resident points hold between calls)
LeaveOutDiag leave_out_diag(const gmb_engine* e, int32_t with_noise) {
  const CovParams& p0 = e->terms[0].cp;
  LeaveOutDiag o{};
  o.noise.sigma2 = p0.sigma2;
  o.noise.mult = p0.noise_tab >= 0 ? p0.noise_mult : nullptr;
  o.noise.cat = p0.noise_tab >= 0 ? e->pts.cat + (int64_t)p0.noise_tab * e->Nr : nullptr;
  o.jitter = p0.jitter;
  o.with_noise = with_noise ? 1 : 0;
  return o;
}

// gmb_loo sums the resident U = L^-T instead of solving: behind a tile-path gradient (U and the refined alpha are this
// factorisation's), unless gmb_set_predict_form(e, 0) asks for the solve.  (Two rows per load: an odd leading dimension -- the
// GMB_LD_PAD probe -- takes the solve.)
bool loo_takes_product_form(const gmb_engine* e) {
  return e->predict_form != 0 && e->fs.live_single() && e->fs.u_resident() && e->fs.gradient_alpha() && e->dUdiag && e->dalpha && e->ld % 2 == 0;
}

// A prediction's workspace for M-tiles of Mt rows, measured against the device before anything is allocated or launched
// (joint_workspace's rule, without the second matrix)
int leave_out_workspace(gmb_engine* e, const char* what, int64_t Mt) {
  Budget need;
  predict_buffers(*e, (double)Mt, need);
  double free_b;
  int rc;
  if ((rc = device_free_bytes(e, &free_b))) return rc;
  if (need.fresh > free_b)
    return fail(e, GMB_ENOMEM, "%s: tiles of %lld rows behind N = %lld need %.0f bytes on the device, %.0f more than it holds for the engine "
                               "now; %.0f bytes are free -- nothing was computed",
                what, (long long)Mt, (long long)e->N, need.total, need.fresh, free_b);
  return predict_workspace(e, Mt);
}

// selection rows (idx, or i0 + j) into the cleared dV (mpad x Np, row index fastest), solved against L: row j = column idx[j] of
// L^-1.  Every block column is solved, also those left of the first selected row, where V is and stays zero: the tile solve has no
// first-column argument, and one schedule serves both.
int leave_out_solve_rows(gmb_engine* e, const int64_t* didx, int64_t i0, int64_t mc, int64_t mpad) {
  HIP_TRY(e, hipMemsetAsync(e->pw.dV, 0, (size_t)(mpad * e->Np) * sizeof(double), e->stream));
  hipLaunchKernelGGL(lo_scatter_kernel, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, e->stream, e->pw.dV, mpad, didx, i0, mc);
  HIP_TRY(e, hipGetLastError());
  return predict_solve_v(e, mpad, false);
}

int loo_impl(gmb_engine* e, int64_t i0, int64_t n, int32_t with_noise, double* mean, double* var, int32_t memspace) {
  int rc = joint_ready(e, "gmb_loo");
  if (rc) return rc;
  if (i0 < 0 || n < 0 || i0 > e->N || n > e->N - i0 || (n > 0 && (!mean || !var)))
    return fail(e, GMB_EINVAL, "gmb_loo: bad range [%lld, %lld + %lld) of N = %lld rows, or null mean/var", (long long)i0, (long long)i0,
                (long long)n, (long long)e->N);
  if (n == 0) return GMB_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const LeaveOutDiag off = leave_out_diag(e, with_noise);
  const CopyKinds ck = copy_kinds(memspace);
  const unsigned nb = (unsigned)((n + 255) / 256);
  if (loo_takes_product_form(e)) {
    const int nct = (int)(e->Np / TILE);
    const int r0 = (int)(i0 / TILE), r1 = (int)((i0 + n - 1) / TILE);
    const int nchunk = (nct - r0 + LOO_CH - 1) / LOO_CH;
    if ((rc = e->dpart.reserve(e->pool, (int64_t)nchunk * e->Np + 2 * n))) return rc;
    reset_predict_timings(e);
    e->tm.predict_gemm_form = 0;
    double* dmean = e->dpart + (int64_t)nchunk * e->Np;
    double* dvar = dmean + n;
    PhaseTimer tp(e);
    auto work = [&]() -> int {
      LooUArgs a{};
      a.U = e->dA;
      a.ldu = e->ld;
      a.udiag = e->dUdiag;
      a.n = e->N;
      a.nct = nct;
      a.r0 = r0;
      a.part = e->dpart;
      a.np = e->Np;
      hipLaunchKernelGGL(loo_u_rowsumsq_kernel, dim3((unsigned)nchunk, (unsigned)(r1 - r0 + 1)), dim3(256), 0, e->stream, a);
      hipLaunchKernelGGL(loo_u_final_kernel, dim3(nb), dim3(256), 0, e->stream, e->dpart, e->Np, nct, i0, n, e->dalpha, e->dy, off, dmean, dvar);
      HIP_TRY(e, hipGetLastError());
      HIP_TRY(e, hipMemcpyAsync(mean, dmean, n * sizeof(double), ck.out, e->stream));
      HIP_TRY(e, hipMemcpyAsync(var, dvar, n * sizeof(double), ck.out, e->stream));
      return GMB_OK;
    };
    return predict_end(e, &tp, work());
  }
  const int64_t Mt = predict_tile_rows(e, n);
  if ((rc = leave_out_workspace(e, "gmb_loo", Mt))) return rc;
  reset_predict_timings(e);
  e->tm.predict_gemm_form = 0;
  const int nchunk = red_chunks(e->N);
  PhaseTimer tp(e);
  auto tiles = [&]() -> int {
    for (int64_t m0 = 0; m0 < n; m0 += Mt) {
      const int64_t mc = std::min<int64_t>(Mt, n - m0);
      const int64_t mpad = round_up(mc, TILE);
      if ((rc = leave_out_solve_rows(e, nullptr, i0 + m0, mc, mpad))) return rc;
      double* pmu = e->dpart;
      double* ps = e->dpart + (int64_t)nchunk * mpad;
      hipLaunchKernelGGL(predict_partial_kernel, dim3((unsigned)(mpad / 256 + (mpad % 256 ? 1 : 0)), nchunk), dim3(256), 0, e->stream,
                         e->pw.dV, mpad, e->dv, e->N, pmu, ps, mpad);
      hipLaunchKernelGGL(loo_solve_final_kernel, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, e->stream, pmu, ps, nchunk, mpad,
                         i0 + m0, mc, e->dy, off, e->pw.dmean, e->pw.dvar);
      HIP_TRY(e, hipGetLastError());
      HIP_TRY(e, hipMemcpyAsync(mean + m0, e->pw.dmean, mc * sizeof(double), ck.out, e->stream));
      HIP_TRY(e, hipMemcpyAsync(var + m0, e->pw.dvar, mc * sizeof(double), ck.out, e->stream));
    }
    return GMB_OK;
  };
  return predict_end(e, &tp, tiles());
}

int leave_out_impl(gmb_engine* e, const int64_t* idx, int64_t m, int32_t with_noise, double* mean, double* var, double* cov, int64_t ldc,
                   int32_t memspace) {
  const char* what = "gmb_leave_out";
  int rc = joint_ready(e, what);
  if (rc) return rc;
  if (!mean || (!var && !cov) || (cov && ldc < m)) return fail(e, GMB_EINVAL, "%s: null mean, neither var nor cov, or ldc < m", what);
  int64_t pos = -1;
  switch (leave_out_check_indices(idx, m, e->N, &pos)) {
    case 0: break;
    case 1: return fail(e, GMB_EINVAL, "%s: idx is null or m = %lld is not in [1, N = %lld]", what, (long long)m, (long long)e->N);
    case 2: return fail(e, GMB_EINVAL, "%s: idx[%lld] = %lld is not a training row (N = %lld)", what, (long long)pos, (long long)idx[pos], (long long)e->N);
    default: return fail(e, GMB_EINVAL, "%s: idx[%lld] = %lld appears twice", what, (long long)pos, (long long)idx[pos]);
  }
  HIP_TRY(e, hipSetDevice(e->device));
  const bool host = memspace != GMB_DEVICE;
  // V (Mr x Np) in the prediction's workspace and C (Mr x Mp) on the joint posterior's second matrix, measured before anything runs
  if ((rc = joint_workspace(e, what, m, false, host && cov ? (double)m * (double)m : 0.0))) return rc;
  ScopedBuf<int64_t> didx(e->pool);
  if ((rc = didx.reserve(e->pool, m))) return rc;
  reset_predict_timings(e);
  e->tm.predict_gemm_form = 0;
  JointState& jt = e->jt;
  const int64_t Mr = jt.Mr, Mp = jt.Mp;
  const LeaveOutDiag off = leave_out_diag(e, with_noise);
  const CopyKinds ck = copy_kinds(memspace);
  const int nchunk = red_chunks(e->N);
  // g = alpha_B and t = X^T g: two vectors in the prepared test points' block, which no launch of this call reads as points
  double* g = e->pw.txs;
  double* t = e->pw.txs + Mr;
  PhaseTimer tp(e);
  auto work = [&]() -> int {
    HIP_TRY(e, hipMemcpyAsync(didx, idx, m * sizeof(int64_t), hipMemcpyHostToDevice, e->stream));
    if ((rc = leave_out_solve_rows(e, didx, 0, m, Mr))) return rc;
    {  // g_j = <V_j, v> = alpha_{idx[j]}
      double* pmu = e->dpart;
      double* ps = e->dpart + (int64_t)nchunk * Mr;
      hipLaunchKernelGGL(predict_partial_kernel, dim3((unsigned)(Mr / 256 + (Mr % 256 ? 1 : 0)), nchunk), dim3(256), 0, e->stream, e->pw.dV,
                         Mr, e->dv, e->N, pmu, ps, Mr);
      hipLaunchKernelGGL(predict_mean_final_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, e->stream, pmu, nchunk, Mr, m, g);
      HIP_TRY(e, hipGetLastError());
    }
    // C = V V^T contracts over all Np columns: those of no training point are cleared first (as joint_covariance does)
    if (e->Np > e->N) HIP_TRY(e, hipMemsetAsync(e->pw.dV + e->N * Mr, 0, (size_t)((e->Np - e->N) * Mr) * sizeof(double), e->stream));
    GemmArgs gc{};
    gc.C = jt.dC;
    gc.ldc = Mr;
    gc.A = e->pw.dV;
    gc.lda = Mr;
    gc.B = e->pw.dV;
    gc.ldb = Mr;
    gc.mt = (int)(Mp / TILE);
    gc.nt = (int)(Mr / TILE);
    gc.k = (int)e->Np;
    gc.alpha = 1.0;
    gc.beta = 0.0;
    gc.tri = 1;
    if ((rc = launch_gemm(e, e->stream, gc, EV_PREDICT_GEMM))) return rc;
    // rows and columns >= m are zero (V is); identity on the padding diagonal, the border row stays zero
    if (Mp > m) hipLaunchKernelGGL(lo_pad_diag_kernel, dim3((unsigned)((Mp - m + 127) / 128)), dim3(128), 0, e->stream, jt.dC, Mr, m, Mp);
    HIP_TRY(e, hipGetLastError());
    if ((rc = joint_factor(e))) {
      if (rc == GMB_ENOTPD)
        return fail(e, GMB_ENOTPD, "%s: (Sigma^-1)_BB of the %lld rows is not positive definite at its row %lld", what, (long long)m, (long long)e->notpd);
      return rc;
    }
    // X = R^-T: identity rows solved against R, in dV (V is dead); what the solve leaves right of column m belongs to no row
    HIP_TRY(e, hipMemsetAsync(e->pw.dV, 0, (size_t)(Mr * Mp) * sizeof(double), e->stream));
    hipLaunchKernelGGL(lo_scatter_kernel, dim3((unsigned)((Mp + 255) / 256)), dim3(256), 0, e->stream, e->pw.dV, Mr, (const int64_t*)nullptr,
                       (int64_t)0, Mp);
    HIP_TRY(e, hipGetLastError());
    if ((rc = trsm_cols(e, e->stream, joint_factor_ref(jt), e->pw.dV, Mr, (int)(Mp / TILE), 0, (int)(Mp / TILE), EV_PREDICT_GEMM, EV_SOLVE_STRIP)))
      return rc;
    if (Mp > m) HIP_TRY(e, hipMemsetAsync(e->pw.dV + m * Mr, 0, (size_t)((Mp - m) * Mr) * sizeof(double), e->stream));
    // t = X^T g, then (X t)_j = (C^-1 g)_j and |X_j|^2 = (C^-1)_jj by the prediction's reduction
    const int nchunk_m = red_chunks(m);
    double* pmu = e->dpart;
    double* ps = e->dpart + (int64_t)nchunk_m * Mp;
    hipLaunchKernelGGL(lo_xt_g_kernel, dim3((unsigned)m), dim3(256), 0, e->stream, e->pw.dV, Mr, g, t);
    hipLaunchKernelGGL(predict_partial_kernel, dim3((unsigned)(Mp / 256 + (Mp % 256 ? 1 : 0)), nchunk_m), dim3(256), 0, e->stream, e->pw.dV, Mr,
                       t, m, pmu, ps, Mp);
    hipLaunchKernelGGL(lo_group_final_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, e->stream, pmu, ps, nchunk_m, Mp, m,
                       (const int64_t*)didx, e->dy, off, e->pw.dmean, e->pw.dvar);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, hipMemcpyAsync(mean, e->pw.dmean, m * sizeof(double), ck.out, e->stream));
    if (var) HIP_TRY(e, hipMemcpyAsync(var, e->pw.dvar, m * sizeof(double), ck.out, e->stream));
    if (!cov) return GMB_OK;
    // C^-1 = X X^T over the factor (dead), symmetrised on its way out, the diagonal corrected there
    GemmArgs gp{};
    gp.C = jt.dC;
    gp.ldc = Mr;
    gp.A = e->pw.dV;
    gp.lda = Mr;
    gp.B = e->pw.dV;
    gp.ldb = Mr;
    gp.mt = (int)(Mp / TILE);
    gp.nt = (int)(Mp / TILE);
    gp.k = (int)Mp;
    gp.alpha = 1.0;
    gp.beta = 0.0;
    gp.tri = 1;
    if ((rc = launch_gemm(e, e->stream, gp, EV_PREDICT_GEMM))) return rc;
    SymArgs sa{};
    sa.C = jt.dC;
    sa.ldc = Mr;
    sa.out = host ? jt.dstage : cov;
    sa.ldo = host ? m : ldc;
    sa.M = m;
    const unsigned nb = (unsigned)((m + 31) / 32);
    hipLaunchKernelGGL(joint_symmetrise_kernel, dim3(nb, nb), dim3(256), 0, e->stream, sa);
    hipLaunchKernelGGL(lo_cov_diag_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, e->stream, sa.out, sa.ldo, m, (const int64_t*)didx, off);
    HIP_TRY(e, hipGetLastError());
    if (host)
      HIP_TRY(e, hipMemcpy2DAsync(cov, ldc * sizeof(double), jt.dstage, m * sizeof(double), m * sizeof(double), m, hipMemcpyDeviceToHost, e->stream));
    return GMB_OK;
  };
  return predict_end(e, &tp, work());
}

// ---- averages of the posterior over groups of points (group_average.hpp) ------------------------------------------------------------

constexpr int64_t GA_TASK_SLAB = 32768;  // tasks per launch (the grid's y extent)

// The partials of `ntask` tasks (a.tasks: the first one's triple, a.part: its row) against a.cols; lists longer than the grid's
// y extent go in slabs.
int launch_group_cov(gmb_engine* e, const GroupCovArgs& a_in, int64_t ntask) {
  const bool gen = a_in.p.n_lin > 0 || a_in.p.n_tab > 0;
  for (int64_t t0 = 0; t0 < ntask; t0 += GA_TASK_SLAB) {
    GroupCovArgs a = a_in;
    a.tasks += 3 * t0;
    a.part += t0 * a.ldp;
    const dim3 grid((unsigned)(a.ldp / GA_COLS), (unsigned)std::min<int64_t>(GA_TASK_SLAB, ntask - t0));
    const bool known = with_kind_nc(a.p.kind, e->nc_pad, [&](auto kind, auto nc) {
      constexpr int K = decltype(kind)::value, NC = decltype(nc)::value;
      auto go = [&](void (*kernel)(GroupCovArgs)) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, e->stream, a); };
      if (gen) go(group_cov_partial_kernel<K, NC, true>);
      else go(group_cov_partial_kernel<K, NC, false>);
    });
    if (!known) return fail(e, GMB_EINVAL, "unknown kernel kind %d", a.p.kind);
    HIP_TRY(e, hipGetLastError());
  }
  return GMB_OK;
}

// what a call's groups come to: tasks (group_tasks.hpp), and the most tasks any row block of 128 groups holds
struct GroupPlan {
  std::vector<int64_t> tasks, first_task;
  int64_t ntask = 0, block_tasks = 0;
};

// Every buffer of gmb_predict_groups, measured against the device before anything is allocated, launched or written
// (joint_workspace's rule): the feature's own workspace -- O(M D), one row block of R and the task partials -- a prediction's for
// Gr = round_up(G + 1, 128) rows (NEVER for M), the product form's second V, and for a covariance the second matrix and the staging
// of a host-side result.
// The buffers are group_buffers' list (workspaces.hpp), walked by the budget and then by the allocation: ONE check, the joint
// posterior's buffers in it.
int group_workspace(gmb_engine* e, const char* what, int64_t M, int64_t G, const GroupPlan& plan, bool gemm_form, bool with_cov, double stage) {
  const int64_t gr = round_up(G + 1, TILE), gp = round_up(G, TILE);
  const double Mp = (double)round_up(M, TILE), Gr = (double)gr, Gp = (double)gp, Np = (double)e->Np;
  auto walk = [&](auto& v) {
    return group_buffers(*e, Mp, (double)G, Gr, Gp, (double)plan.ntask, (double)plan.block_tasks, gemm_form, with_cov, stage, v);
  };
  Budget need;
  walk(need);
  double free_b;
  int rc;
  if ((rc = device_free_bytes(e, &free_b))) return rc;
  // (every grid extent and index below stays inside 31 bits with these)
  if (need.fresh > free_b || Mp > 1073741824.0 || Gr * ((Np > Mp ? Np : Mp) / 256.0 + 1.0) > 2147483647.0)
    return fail(e, GMB_ENOMEM, "%s: M = %lld points in G = %lld groups behind N = %lld needs %.0f bytes on the device (points and R: %.0f, "
                               "task partials: %.0f, V: %.0f%s, C: %.0f), %.0f more than it holds for the engine now; %.0f bytes are free -- "
                               "nothing was computed",
                what, (long long)M, (long long)G, (long long)e->N, need.total, e->ga.bytes(Mp, e->D),
                sizeof(double) * group_partial_elems((double)plan.ntask, (double)plan.block_tasks, Np, Mp), e->pw2.bytes(Gr, e->Np),
                gemm_form ? " twice" : "", with_cov ? sizeof(double) * joint_matrix_elems(Gr, Gp) : 0.0, need.fresh, free_b);
  Reserver take{e->pool};
  walk(take);
  return take.rc || !with_cov ? take.rc : joint_fixed_buffers(e, G, gr, gp);
}

int predict_groups_sel(gmb_engine* e, const uint32_t* sel, const char* what, const double* Xs, int64_t M, int64_t ldxs, const int64_t* offsets,
                       int64_t G, const double* weights, double* mean, double* var, double* cov, int64_t ldc, int32_t memspace) {
  int rc = joint_ready(e, what);
  if (rc) return rc;
  uint32_t terms;
  if ((rc = resolve_terms(e, sel, what, &terms))) return rc;
  if (!Xs || !offsets || !mean || (!var && !cov) || G < 1 || M < 1 || ldxs < e->D || (cov && ldc < G))
    return fail(e, GMB_EINVAL, "%s: null Xs/offsets/mean, neither var nor cov, G < 1, M < 1, ldxs < D or ldc < G", what);
  int64_t pos = -1;
  switch (group_check_offsets(offsets, G, M, &pos)) {
    case 0: break;
    case 2: return fail(e, GMB_EINVAL, "%s: offsets[0] = %lld, not 0", what, (long long)offsets[0]);
    case 3:
      return fail(e, GMB_EINVAL, "%s: group %lld is empty or runs backwards (offsets[%lld] = %lld, offsets[%lld] = %lld)", what, (long long)pos,
                  (long long)pos, (long long)offsets[pos], (long long)pos + 1, (long long)offsets[pos + 1]);
    case 4: return fail(e, GMB_EINVAL, "%s: offsets[G] = %lld, not M = %lld", what, (long long)offsets[G], (long long)M);
    default: return fail(e, GMB_EINVAL, "%s: bad offsets", what);
  }
  const bool host = memspace != GMB_DEVICE;
  if (weights && host)
    for (int64_t m = 0; m < M; ++m)
      if (!std::isfinite(weights[m])) return fail(e, GMB_EINVAL, "%s: weights[%lld] is not finite", what, (long long)m);
  HIP_TRY(e, hipSetDevice(e->device));

  if (M > 1073741824)
    return fail(e, GMB_ENOMEM, "%s: M = %lld points are more than a call takes (2^30) -- nothing was computed", what, (long long)M);
  GroupPlan plan;
  plan.ntask = group_build_tasks(offsets, G, GROUP_CHUNK, &plan.tasks, &plan.first_task);
  for (int64_t g0 = 0; g0 < G; g0 += GA_ROWS)
    plan.block_tasks = std::max(plan.block_tasks, plan.first_task[std::min<int64_t>(G, g0 + GA_ROWS)] - plan.first_task[g0]);
  const bool gemm_form = predict_takes_gemm_form(e);
  if ((rc = group_workspace(e, what, M, G, plan, gemm_form, cov != nullptr, host && cov ? (double)G * (double)G : 0.0))) return rc;
  std::vector<double> mean_w;  // weights == NULL: 1 / |g|, a plain mean (alive until the call's stream has drained)
  if (!weights) {
    mean_w.resize((size_t)M);
    for (int64_t g = 0; g < G; ++g) {
      const double wg = 1.0 / (double)(offsets[g + 1] - offsets[g]);
      for (int64_t m = offsets[g]; m < offsets[g + 1]; ++m) mean_w[(size_t)m] = wg;
    }
  }
  reset_predict_timings(e);
  e->tm.predict_gemm_form = gemm_form ? 1 : 0;

  JointState& jt = e->jt;
  const int64_t Mp = round_up(M, TILE), Gr = round_up(G + 1, TILE), Gp = round_up(G, TILE);
  const CopyKinds ck = copy_kinds(memspace);
  const int64_t* d_tasks = e->ga_idx;
  const int64_t* d_first = e->ga_idx + 3 * plan.ntask;
  const int64_t* d_off = d_first + (G + 1);
  const PointSet pts{e->ga.xs, e->ga.xl, e->ga.cat, M, Mp};
  const int t_first = first_term(terms);
  PhaseTimer tp(e);
  auto work = [&]() -> int {
    HIP_TRY(e, hipMemcpy2DAsync(e->ga.Xs, e->D * sizeof(double), Xs, ldxs * sizeof(double), e->D * sizeof(double), M, ck.in, e->stream));
    if (weights) HIP_TRY(e, hipMemcpyAsync(e->ga.w, weights, M * sizeof(double), ck.in, e->stream));
    else HIP_TRY(e, hipMemcpyAsync(e->ga.w, mean_w.data(), M * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(e->ga_idx, plan.tasks.data(), 3 * plan.ntask * sizeof(int64_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(e->ga_idx + 3 * plan.ntask, plan.first_task.data(), (G + 1) * sizeof(int64_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(e->ga_idx + 3 * plan.ntask + (G + 1), offsets, (G + 1) * sizeof(int64_t), hipMemcpyHostToDevice, e->stream));
    // A's rows G .. Gr - 1 belong to no group and stay zero; C starts as the bordered layout's padding (identity on the padding
    // diagonal, a zero border row)
    HIP_TRY(e, hipMemsetAsync(e->pw.dV, 0, (size_t)(Gr * e->Np) * sizeof(double), e->stream));
    if (cov) {
      HIP_TRY(e, hipMemsetAsync(jt.dC, 0, (size_t)(Gr * Gp) * sizeof(double), e->stream));
      if (Gp > G) hipLaunchKernelGGL(lo_pad_diag_kernel, dim3((unsigned)((Gp - G + 127) / 128)), dim3(128), 0, e->stream, jt.dC, Gr, G, Gp);
      HIP_TRY(e, hipGetLastError());
    }
    rc = walk_terms(e, terms, [&](int t) -> int {
      const gmb_engine::Term& tr = e->terms[t];
      const bool first = t == t_first;
      int r;
      if ((r = prep_points(e, e->ga.Xs, M, e->D, Mp, e->ga.xs, e->ga.xl, e->ga.cat, &tr.pa))) return r;
      GroupCovArgs a{};
      a.p = tr.cp;
      a.pts = pts;
      a.w = e->ga.w;
      a.part = e->ga_part;
      a.offsets = d_off;
      GroupFinishArgs f{};
      f.part = e->ga_part;
      f.first_task = d_first;
      f.accumulate = first ? 0 : 1;
      f.offsets = d_off;
      // A: every task against the training points -> dV (Gr x Np, group index fastest; columns >= N are zero)
      a.cols = train_set(e);
      a.tasks = d_tasks;
      a.ldp = e->Np;
      ev_begin(e, e->stream, EV_GROUP_COV, 0.0, (int)(a.ldp / GA_COLS), (int)plan.ntask, 0, 0);
      r = launch_group_cov(e, a, plan.ntask);
      ev_end(e);
      if (r) return r;
      f.ldp = e->Np;
      f.task0 = 0;
      f.g0 = 0;
      f.ng = G;
      f.ncols = e->Np;
      f.out = e->pw.dV;
      f.ldo = Gr;
      hipLaunchKernelGGL(group_cov_finish_kernel, dim3((unsigned)(G * ((e->Np + 255) / 256))), dim3(256), 0, e->stream, f);
      HIP_TRY(e, hipGetLastError());
      // Q: the group points against themselves, a row block of 128 groups at a time -> R -> folded into C (and kss)
      a.cols = pts;
      a.ldp = Mp;
      a.diag_only = cov ? 0 : 1;
      f.ldp = Mp;
      f.ncols = M;
      f.out = e->ga.R;
      f.ldo = GA_ROWS;
      f.accumulate = 0;
      f.diag_only = a.diag_only;
      for (int64_t g0 = 0; g0 < G; g0 += GA_ROWS) {
        const int64_t ng = std::min<int64_t>(GA_ROWS, G - g0);
        const int64_t tb0 = plan.first_task[g0], nt = plan.first_task[g0 + ng] - tb0;
        a.tasks = d_tasks + 3 * tb0;
        ev_begin(e, e->stream, EV_GROUP_COV, 0.0, (int)(a.ldp / GA_COLS), (int)nt, 0, a.diag_only ? 2 : 1);
        r = launch_group_cov(e, a, nt);
        ev_end(e);
        if (r) return r;
        f.task0 = tb0;
        f.g0 = g0;
        f.ng = ng;
        hipLaunchKernelGGL(group_cov_finish_kernel, dim3((unsigned)(ng * ((M + 255) / 256))), dim3(256), 0, e->stream, f);
        GroupFoldArgs fo{};
        fo.R = e->ga.R;
        fo.w = e->ga.w;
        fo.offsets = d_off;
        fo.g0 = g0;
        fo.G = G;
        fo.C = cov ? (double*)jt.dC : nullptr;
        fo.ldc = Gr;
        fo.kss = e->pw.dkss;
        fo.accumulate = first ? 0 : 1;
        fo.diag_only = a.diag_only;
        hipLaunchKernelGGL(group_fold_kernel, dim3((unsigned)(a.diag_only ? 1 : g0 + ng)), dim3(GA_ROWS), 0, e->stream, fo);
        HIP_TRY(e, hipGetLastError());
      }
      return GMB_OK;
    });
    if (rc) return rc;
    // from here on it is a prediction at Gr rows: V_A = A L^-T, mean = V_A v, var = diag Q - |V_A|^2 (not clipped)
    if ((rc = predict_solve_v(e, Gr, gemm_form))) return rc;
    if ((rc = predict_reduce(e, G, Gr, gemm_form))) return rc;
    HIP_TRY(e, hipMemcpyAsync(mean, e->pw.dmean, G * sizeof(double), ck.out, e->stream));
    if (var) HIP_TRY(e, hipMemcpyAsync(var, e->pw.dvar, G * sizeof(double), ck.out, e->stream));
    if (!cov) return GMB_OK;
    // C -= V_A V_A^T as joint_covariance does it: the product form's V turned into the update's k-major layout, the columns of no
    // training point cleared, the trailing update's launch with contraction length Np
    if (gemm_form && (rc = launch_transpose(e, e->stream, e->pw2.dV2, e->Np, e->pw.dV, Gr, (int)e->Np, (int)Gr))) return rc;
    if (e->Np > e->N) HIP_TRY(e, hipMemsetAsync(e->pw.dV + e->N * Gr, 0, (size_t)((e->Np - e->N) * Gr) * sizeof(double), e->stream));
    GemmArgs g{};
    g.C = jt.dC;
    g.ldc = Gr;
    g.A = e->pw.dV;
    g.lda = Gr;
    g.B = e->pw.dV;
    g.ldb = Gr;
    g.mt = (int)(Gp / TILE);
    g.nt = (int)(Gr / TILE);
    g.k = (int)e->Np;
    g.alpha = -1.0;
    g.beta = 1.0;
    g.tri = 1;
    if ((rc = launch_gemm(e, e->stream, g, EV_PREDICT_GEMM))) return rc;
    // both triangles from the lower one (exactly symmetric), the reduction's variance on the diagonal (cov's diagonal IS var)
    SymArgs sa{};
    sa.C = jt.dC;
    sa.ldc = Gr;
    sa.out = host ? (double*)jt.dstage : cov;
    sa.ldo = host ? G : ldc;
    sa.M = G;
    const unsigned nb = (unsigned)((G + 31) / 32);
    hipLaunchKernelGGL(joint_symmetrise_kernel, dim3(nb, nb), dim3(256), 0, e->stream, sa);
    hipLaunchKernelGGL(group_cov_diag_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, e->stream, sa.out, sa.ldo, G, (const double*)e->pw.dvar);
    HIP_TRY(e, hipGetLastError());
    if (host)
      HIP_TRY(e, hipMemcpy2DAsync(cov, ldc * sizeof(double), jt.dstage, G * sizeof(double), G * sizeof(double), G, hipMemcpyDeviceToHost, e->stream));
    return GMB_OK;
  };
  return predict_end(e, &tp, work());
}

// ---- a batch of experiments by greedy integrated variance reduction (design_batch.hpp) ----------------------------

// Every buffer of gmb_design_batch, measured against the device before anything is allocated, launched, written or -- the caller's
// arrays included -- read (joint_workspace's rule).  The buffers are design_buffers' list (workspaces.hpp), walked by this budget
// and then by design_reserve: a prediction's for the plan's largest point tile, the product form's second V, and the feature's
// own workspace.
int design_measure(gmb_engine* e, const char* what, const DesignPlan& pl, int64_t q, bool gemm_form) {
  Budget need;
  design_buffers(*e, pl, (double)DesignPlan::result_doubles(pl.M, q), gemm_form, need);
  double free_b;
  int rc;
  if ((rc = device_free_bytes(e, &free_b))) return rc;
  if (need.fresh > free_b)
    return fail(e, GMB_ENOMEM, "%s: M = %lld candidates and R = %lld reference points behind N = %lld need %.0f bytes on the device (D: %.0f, "
                               "the candidates' solved rows: %.0f, V of one point tile: %.0f%s), %.0f more than it holds for the engine now; "
                               "%.0f bytes are free -- nothing was computed",
                what, (long long)pl.M, (long long)pl.R, (long long)e->N, need.total, 8.0 * (double)pl.Mc * (double)pl.ld,
                8.0 * (double)pl.Mc * (double)e->Np, e->pw2.bytes((double)pl.mt, e->Np), gemm_form ? " twice" : "", need.fresh, free_b);
  return GMB_OK;
}
int design_reserve(gmb_engine* e, const DesignPlan& pl, int64_t q, bool gemm_form) {
  Reserver take{e->pool};
  design_buffers(*e, pl, (double)DesignPlan::result_doubles(pl.M, q), gemm_form, take);
  return take.rc;
}

// `n` points of the caller's (host, or device: copied to the host first) must hold no NaN; 0, or the refusal
int design_check_points(gmb_engine* e, const char* what, const char* name, const double* X, int64_t n, int64_t ldx, bool host,
                        std::vector<double>& scratch) {
  const int64_t D = e->D;
  const double* src = X;
  int64_t l = ldx;
  if (!host) {
    scratch.resize((size_t)(n * D));
    HIP_TRY(e, hipMemcpy2DAsync(scratch.data(), D * sizeof(double), X, ldx * sizeof(double), D * sizeof(double), n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    src = scratch.data();
    l = D;
  }
  for (int64_t i = 0; i < n; ++i)
    for (int64_t d = 0; d < D; ++d)
      if (std::isnan(src[i * l + d])) return fail(e, GMB_EINVAL, "%s: %s[%lld, %lld] is NaN", what, name, (long long)i, (long long)d);
  return GMB_OK;
}

int design_batch_impl(gmb_engine* e, const double* Xc, int64_t M, int64_t ldc, const double* Xr, int64_t R, int64_t ldr, const double* w,
                      int32_t q, int32_t with_noise, int32_t allow_repeats, int64_t* picks, double* gains, double* score0, double* ivar0,
                      int32_t memspace) {
  const char* what = "gmb_design_batch";
  int rc = joint_ready(e, what);
  if (rc) return rc;
  if (M < 1 || R < 1 || q < 0)
    return fail(e, GMB_EINVAL, "%s: M = %lld candidates, R = %lld reference points, q = %d picks (M >= 1, R >= 1 and q >= 0 are required)", what,
                (long long)M, (long long)R, (int)q);
  if (!Xc || !Xr || ldc < e->D || ldr < e->D || (q > 0 && (!picks || !gains)))
    return fail(e, GMB_EINVAL, "%s: null Xc/Xr, ldc < D, ldr < D, or q > 0 without picks/gains", what);
  HIP_TRY(e, hipSetDevice(e->device));
  const bool host = memspace != GMB_DEVICE;
  const CopyKinds ck = copy_kinds(memspace);

  // the plan first (host arithmetic), then the bytes against the device, then the arguments' values, then the allocation: a
  // refusal has touched nothing
  DesignPlan pl;
  switch (pl.make(e->Np, M, R)) {
    case 0: break;
    case 4:
      return fail(e, GMB_ENOMEM, "%s: M = %lld candidates are more than one M-tile of a prediction holds behind N = %lld (%lld rows: their "
                                 "solved rows alone would take %.0f bytes) -- nothing was computed",
                  what, (long long)M, (long long)e->N, (long long)pl.mt_max, 8.0 * (double)M * (double)e->Np);
    default:
      return fail(e, GMB_ENOMEM, "%s: R = %lld reference points are more than a call takes (2^30) -- nothing was computed", what, (long long)R);
  }
  const bool gemm_form = predict_takes_gemm_form(e);
  if ((rc = design_measure(e, what, pl, q, gemm_form))) return rc;
  std::vector<double> scratch, hw;
  if ((rc = design_check_points(e, what, "Xc", Xc, M, ldc, host, scratch))) return rc;
  if ((rc = design_check_points(e, what, "Xr", Xr, R, ldr, host, scratch))) return rc;
  if (w) {
    const double* src = w;
    if (!host) {
      hw.resize((size_t)R);
      HIP_TRY(e, hipMemcpyAsync(hw.data(), w, R * sizeof(double), hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(e, hipStreamSynchronize(e->stream));
      src = hw.data();
    }
    for (int64_t r = 0; r < R; ++r)
      if (!(src[r] >= 0.0) || !std::isfinite(src[r]))
        return fail(e, GMB_EINVAL, "%s: weights[%lld] = %g is negative or not finite", what, (long long)r, src[r]);
  } else {
    hw.assign((size_t)R, 1.0 / (double)R);
  }
  if ((rc = design_reserve(e, pl, q, gemm_form))) return rc;
  reset_predict_timings(e);
  e->tm.predict_gemm_form = gemm_form ? 1 : 0;

  DesignWorkspace& z = e->dz;
  const int64_t Mc = pl.Mc, ld = pl.ld;
  const int64_t nres = DesignPlan::result_doubles(M, q);
  double* d_gains = z.res;
  double* d_score = z.res + q;
  double* d_ivar = d_score + M;
  int64_t* d_picks = reinterpret_cast<int64_t*>(d_ivar + 1);
  const uint32_t terms = all_terms_mask(e);
  const int nterms = (int)e->terms.size();
  const int t_first = first_term(terms);
  const PointSet cand{z.xs, z.xl, z.cat, M, Mc};
  std::vector<double> hres(host ? (size_t)nres : 0);
  PhaseTimer tp(e);
  // (while profiling: the call's phases as trace lines of their own, around the launches' -- kind 20)
  auto phase_open = [&](int which, int k) -> size_t {
    if (!e->profiling) return (size_t)-1;
    ev_begin(e, e->stream, EV_DESIGN, 0.0, (int)M, (int)ld, k, which);
    return e->evs.size() - 1;
  };
  auto phase_close = [&](size_t at) {
    if (at != (size_t)-1) (void)hipEventRecord(e->evs[at].b, e->evs[at].s);
  };
  auto work = [&]() -> int {
    HIP_TRY(e, hipMemsetAsync(z.w, 0, (size_t)ld * sizeof(double), e->stream));
    HIP_TRY(e, hipMemsetAsync(z.var, 0, (size_t)ld * sizeof(double), e->stream));
    HIP_TRY(e, hipMemsetAsync(z.dpiv, 0, (size_t)ld * sizeof(double), e->stream));
    HIP_TRY(e, hipMemsetAsync(z.ctl, 0, (size_t)DesignPlan::DESIGN_CTL_DOUBLES * sizeof(double), e->stream));
    HIP_TRY(e, hipMemsetAsync(z.mask, 0, (size_t)Mc * sizeof(int32_t), e->stream));
    HIP_TRY(e, hipMemsetAsync(z.res, 0, (size_t)nres * sizeof(double), e->stream));
    if (w) HIP_TRY(e, hipMemcpyAsync(z.w + Mc, w, R * sizeof(double), ck.in, e->stream));
    else HIP_TRY(e, hipMemcpyAsync(z.w + Mc, hw.data(), R * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpy2DAsync(z.Xs, e->D * sizeof(double), Xc, ldc * sizeof(double), e->D * sizeof(double), M, ck.in, e->stream));
    // the candidates as the first term reads them: the noise a prediction would add, by kss_kernel's own term
    int r;
    if ((r = prep_points(e, z.Xs, M, e->D, Mc, z.xs, z.xl, z.cat, &e->terms[t_first].pa))) return r;
    DesignNoiseArgs na{};
    na.p = first_pass_params(e, t_first);
    na.pts = cand;
    na.with_noise = with_noise;
    na.noise = z.noise;
    hipLaunchKernelGGL(design_noise_kernel, dim3((unsigned)((Mc + 255) / 256)), dim3(256), 0, e->stream, na);
    HIP_TRY(e, hipGetLastError());

    for (int64_t ti = 0; ti < pl.ntile; ++ti) {
      const DesignTile tl = pl.tile(ti);
      const double* X = ti == 0 ? Xc : Xr + (tl.first - M) * ldr;
      // 1. V = L^-1 K(X, P_tile) in the form a prediction would take, and the latent variances by its own reduction
      size_t ph = phase_open(0, 0);
      if ((r = predict_cross_cov(e, terms, X, tl.count, tl.mpad, ti == 0 ? ldc : ldr, 0, ck.in))) return r;
      if ((r = predict_solve_v(e, tl.mpad, gemm_form))) return r;
      if ((r = predict_reduce(e, tl.count, tl.mpad, gemm_form))) return r;
      if (ti > 0) HIP_TRY(e, hipMemcpyAsync(z.var + tl.col0, e->pw.dvar, tl.count * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      // (as joint_covariance: the product form's V into the update's k-major layout, the columns of no training point cleared)
      if (gemm_form && (r = launch_transpose(e, e->stream, e->pw2.dV2, e->Np, e->pw.dV, tl.mpad, (int)e->Np, (int)tl.mpad))) return r;
      if (e->Np > e->N)
        HIP_TRY(e, hipMemsetAsync(e->pw.dV + e->N * tl.mpad, 0, (size_t)((e->Np - e->N) * tl.mpad) * sizeof(double), e->stream));
      if (ti == 0) HIP_TRY(e, hipMemcpyAsync(z.dVc, e->pw.dV, (size_t)(Mc * e->Np) * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      phase_close(ph);
      ph = phase_open(1, 0);
      // 2. the prior K(Xc, P_tile) into D's columns of the tile, term by term; both point sets are workspace copies (a model of
      // one term builds on the preparations as they stand)
      const PointSet tile_pts{e->pw.txs, e->pw.txl, e->pw.tcat, tl.count, tl.mpad};
      bool first = true;
      for (int t = 0; t < nterms; ++t) {
        if (!((terms >> t) & 1u)) continue;
        if (nterms > 1) {
          if ((r = prep_points(e, e->pw.dXs, tl.count, e->D, tl.mpad, e->pw.txs, e->pw.txl, e->pw.tcat, &e->terms[t].pa))) return r;
          if ((r = prep_points(e, z.Xs, M, e->D, Mc, z.xs, z.xl, z.cat, &e->terms[t].pa))) return r;
        }
        CovTileArgs a{};
        a.p = e->terms[t].cp;
        a.rows = tile_pts;
        a.cols = cand;
        a.out = z.dD + tl.col0;
        a.ldo = ld;
        a.ti = (int)(tl.mpad / TILE);
        a.tj = (int)(Mc / TILE);
        a.mode = COV_CROSS;
        a.accumulate = first ? 0 : 1;
        if ((r = launch_cov(e, a))) return r;
        first = false;
      }
      // 3. D[:, tile] -= Vc V_tile^T: the joint posterior's update with contraction length Np
      GemmArgs g{};
      g.C = z.dD + tl.col0;
      g.ldc = ld;
      g.A = z.dVc;
      g.lda = Mc;
      g.B = e->pw.dV;
      g.ldb = tl.mpad;
      g.mt = (int)(Mc / TILE);
      g.nt = (int)(tl.mpad / TILE);
      g.k = (int)e->Np;
      g.alpha = -1.0;
      g.beta = 1.0;
      if ((r = launch_gemm(e, e->stream, g, EV_PREDICT_GEMM))) return r;
      phase_close(ph);
    }
    hipLaunchKernelGGL(design_ivar_kernel, dim3(1), dim3(DESIGN_PICK_THREADS), 0, e->stream, (const double*)z.w, (const double*)z.var, ld, d_ivar);
    HIP_TRY(e, hipGetLastError());

    // 4. the greedy loop: step (the downdate of the last pick, the sums of the new score) and pick, back to back
    if (q > 0 || score0) {
      DesignStepArgs sa{};
      sa.D = z.dD;
      sa.ld = ld;
      sa.M = M;
      sa.Mc = Mc;
      sa.piv = z.dpiv;
      sa.w = z.w;
      sa.ctl = z.ctl;
      sa.part = z.part;
      DesignPickArgs pa{};
      pa.D = z.dD;
      pa.ld = ld;
      pa.M = M;
      pa.Mc = Mc;
      pa.nchunk = pl.nchunk;
      pa.part = z.part;
      pa.noise = z.noise;
      pa.mask = z.mask;
      pa.ctl = z.ctl;
      pa.piv = z.dpiv;
      pa.gains = d_gains;
      pa.picks = d_picks;
      pa.score0 = d_score;
      pa.allow_repeats = allow_repeats;
      pa.score_only = q == 0 ? 1 : 0;
      const dim3 sgrid((unsigned)pl.nchunk, (unsigned)((M + DESIGN_ROWS - 1) / DESIGN_ROWS));
      const size_t ph = phase_open(2, (int)q);
      for (int32_t t = 0; t < (q > 0 ? q : 1); ++t) {
        hipLaunchKernelGGL(design_step_kernel, sgrid, dim3(DESIGN_THREADS), 0, e->stream, sa);
        pa.t = t;
        hipLaunchKernelGGL(design_pick_kernel, dim3(1), dim3(DESIGN_PICK_THREADS), 0, e->stream, pa);
      }
      phase_close(ph);
      HIP_TRY(e, hipGetLastError());
    }
    // 5. the results
    if (host) {
      HIP_TRY(e, hipMemcpyAsync(hres.data(), z.res, (size_t)nres * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    } else {
      if (q > 0) HIP_TRY(e, hipMemcpyAsync(gains, d_gains, q * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      if (q > 0) HIP_TRY(e, hipMemcpyAsync(picks, d_picks, q * sizeof(int64_t), hipMemcpyDeviceToDevice, e->stream));
      if (score0) HIP_TRY(e, hipMemcpyAsync(score0, d_score, M * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      if (ivar0) HIP_TRY(e, hipMemcpyAsync(ivar0, d_ivar, sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    }
    return GMB_OK;
  };
  if ((rc = predict_end(e, &tp, work()))) return rc;
  if (host) {
    if (q > 0) std::memcpy(gains, hres.data(), (size_t)q * sizeof(double));
    if (q > 0) std::memcpy(picks, hres.data() + q + M + 1, (size_t)q * sizeof(int64_t));
    if (score0) std::memcpy(score0, hres.data() + q, (size_t)M * sizeof(double));
    if (ivar0) *ivar0 = hres[(size_t)(q + M)];
  }
  return GMB_OK;
}

// ---- the sparse (FITC) path: fitc.hpp, fitc_plan.hpp, DESIGN 3.17 ------------------------------------------------------------------
// The inducing points stand where the training set stands in a prediction: K(X-tile, Z) is the cross-covariance launch, A^T the
// triangular solve against Lu, the two m x m factors go through chol_factor as matrices of their own (as the joint posterior's C
// does).  Nothing of the exact path is touched: the factor buffer, dW, the prediction workspaces stay as they are (and unallocated
// if they were); theta is set as gmb_set_theta sets it, so a resident exact factor is stale afterwards by FactorState's own rules.

FactorRef fitc_factor_u(FitcState& s) { return FactorRef{s.dKuu, s.mr, s.m, s.mp, s.mr, s.dDinvU, s.dscalU, &s.dctU}; }
FactorRef fitc_factor_b(FitcState& s) { return FactorRef{s.dB, s.mr, s.m, s.mp, s.mr, s.dDinvB, s.dscalB, &s.dctB}; }
PointSet fitc_z_set(const FitcState& s) { return PointSet{s.zpts.xs, s.zpts.xl, s.zpts.cat, s.m, s.mr}; }

// the models the sparse path is built for
int fitc_scope(gmb_engine* e, const char* what) {
  const gmb_kernel_spec& sp = e->spec;
  if (sp.n_coreg != 0 || sp.out_col >= 0)
    return fail(e, GMB_EINVAL, "%s: the sparse approximation supports one output and no categorical dimensions (n_coreg = %d, out_col = %d)",
                what, sp.n_coreg, sp.out_col);
  if (sp.additive) return fail(e, GMB_EINVAL, "%s: the sparse approximation does not support additive models", what);
  if (sp.n_lin != 0) return fail(e, GMB_EINVAL, "%s: the sparse approximation does not support linear dimensions (n_lin = %d)", what, sp.n_lin);
  if (e->periodic != 0) return fail(e, GMB_EINVAL, "%s: the sparse approximation does not support periodic kernels", what);
  if (e->solve_hook || e->dist_mode != 0)
    return fail(e, GMB_EINVAL, "%s is not available on distributed engines (gmb_dist_*, capacity mode)", what);
  return GMB_OK;
}

int fitc_plan_for(gmb_engine* e, const char* what, int64_t m, FitcPlan* pl) {
  switch (pl->make(e->N, m)) {
    case 0: return GMB_OK;
    case 2: return fail(e, GMB_EINVAL, "%s: m = %lld inducing points (at least 1)", what, (long long)m);
    case 3: return fail(e, GMB_EINVAL, "%s: m = %lld inducing points exceed the limit of %lld", what, (long long)m, (long long)FITC_MAX_M);
    default: return fail(e, GMB_EINVAL, "%s: N = %lld is out of range", what, (long long)e->N);
  }
}

// measure a list of buffers against the device, then allocate it (`list(v)`: one of workspaces.hpp's fitc_*_buffers over a visitor)
template <typename List>
int fitc_reserve(gmb_engine* e, const char* what, const FitcPlan& pl, List&& list) {
  Budget need;
  list(need);
  double free_b;
  int rc;
  if ((rc = device_free_bytes(e, &free_b))) return rc;
  if (need.fresh > free_b)
    return fail(e, GMB_ENOMEM, "%s: N = %lld with m = %lld inducing points needs %.0f bytes on the device (m x m: %.0f each, an m x tile block of "
                               "%lld columns: %.0f), %.0f more than the engine holds now; %.0f bytes are free -- nothing was computed",
                what, (long long)pl.N, (long long)pl.m, need.total, 8.0 * (double)pl.mr * (double)pl.mp, (long long)pl.tmax,
                8.0 * (double)pl.mr * (double)pl.tmax, need.fresh, free_b);
  Reserver take{e->pool};
  list(take);
  return take.rc;
}

int fitc_set_inducing_impl(gmb_engine* e, const double* Z, int64_t m, int64_t ldz, int32_t memspace) {
  const char* what = "gmb_fitc_set_inducing";
  if (!e) return GMB_EINVAL;
  FitcState& s = e->fitc;
  s.drop_inducing();
  if (e->N <= 0) return fail(e, GMB_EINVAL, "gmb_set_data must precede %s", what);
  if (!e->have_spec) return fail(e, GMB_EINVAL, "gmb_set_kernel must precede %s", what);
  int rc = fitc_scope(e, what);
  if (rc) return rc;
  if (!Z || ldz < e->D) return fail(e, GMB_EINVAL, "%s: bad Z/ldz", what);
  FitcPlan pl;
  if ((rc = fitc_plan_for(e, what, m, &pl))) return rc;
  if (memspace != GMB_DEVICE)
    for (int64_t i = 0; i < m; ++i)
      for (int c = 0; c < e->D; ++c)
        if (!std::isfinite(Z[i * ldz + c])) return fail(e, GMB_EINVAL, "%s: Z[%lld, %d] is not finite", what, (long long)i, c);
  HIP_TRY(e, hipSetDevice(e->device));
  const int D = e->D;
  if ((rc = fitc_reserve(e, what, pl, [&](auto& v) { return fitc_fixed_buffers(s, pl, D, v); }))) return rc;
  const hipMemcpyKind kind = memspace == GMB_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIP_TRY(e, hipMemcpy2DAsync(s.dZ, D * sizeof(double), Z, ldz * sizeof(double), D * sizeof(double), m, kind, e->stream));
  HIP_TRY(e, hipMemsetAsync(s.dzero, 0, (size_t)pl.mr * sizeof(double), e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  s.m = pl.m, s.mp = pl.mp, s.mr = pl.mr;
  s.have_z = true;
  return GMB_OK;
}

// K(P, Z) for the prepared points P (padded to `pad` rows) into V (pad x mp, P's index fastest)
int fitc_cross_cov(gmb_engine* e, const PointSet& rows, int64_t pad, double* V) {
  const FitcState& s = e->fitc;
  CovTileArgs a{};
  a.p = e->terms[0].cp;
  a.rows = rows;
  a.cols = fitc_z_set(s);
  a.out = V;
  a.ldo = pad;
  a.ti = (int)(pad / TILE);
  a.tj = (int)(s.mp / TILE);
  a.mode = COV_CROSS;
  ev_begin(e, e->stream, EV_FITC, 0.0, a.ti, a.tj, 0, 0);
  const int rc = launch_cov(e, a);
  ev_end(e);
  return rc;
}

// V <- V L^-T (pad rows): the blocked solve of a prediction.  The columns m .. mp - 1 belong to no inducing point and the border
// row of the factor reaches them: cleared, as the joint posterior clears them.
int fitc_solve_lt(gmb_engine* e, const FactorRef& f, double* V, int64_t pad) {
  int rc = trsm_cols(e, e->stream, f, V, pad, (int)(pad / TILE), 0, (int)(f.Np / TILE), EV_CHOL_SOLVE_GEMM, EV_SOLVE_STRIP);
  if (rc) return rc;
  if (f.Np > f.N) HIP_TRY(e, hipMemsetAsync(V + f.N * pad, 0, (size_t)((f.Np - f.N) * pad) * sizeof(double), e->stream));
  return GMB_OK;
}

// V <- V L^-1 (pad rows): the second triangular pass of gmb_predict_with_grad, on this factor
int fitc_solve_l(gmb_engine* e, const FactorRef& f, double* V, int64_t pad) {
  const TriOperand L{f.A, f.ld, f.A, f.ld, (int64_t)TILE * (f.ld + 1)};
  const int nb = (int)(f.Np / TILE);
  ev_begin(e, e->stream, EV_FITC, (double)pad * (double)f.N * (double)f.N, (int)(pad / TILE), nb, 0, 1);
  for (int b = nb - 1; b >= 0; --b) {
    hipLaunchKernelGGL(vsolve_diag_kernel, dim3((unsigned)(pad / VS_ROWS)), dim3(VS_ROWS), 0, e->stream, L, (int64_t)b, f.N, V, pad);
    if (b > 0)
      hipLaunchKernelGGL(vsolve_update_kernel, dim3((unsigned)(pad / VS_PTS), (unsigned)b), dim3(256), 0, e->stream, L, (int64_t)b, f.N, V, pad);
  }
  ev_end(e);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// one of the two m x m factorisations, by the schedule chol_factor gives a matrix of its size; synchronises and looks at the result
int fitc_factor(gmb_engine* e, const FactorRef& f, const char* which) {
  HIP_TRY(e, hipMemsetAsync(f.scal, 0, (size_t)SCAL_GACC_AT * sizeof(double), e->stream));
  CholResult res;
  int rc = chol_factor(e, f, CholOpts{}, &res);
  if (rc) return rc;
  int32_t info = 0;
  uint32_t ab = 0;
  HIP_TRY(e, hipMemcpyAsync(&info, f.info(), sizeof info, hipMemcpyDeviceToHost, e->stream));
  if (res.tiles) HIP_TRY(e, hipMemcpyAsync(&ab, *f.ct + 1, sizeof ab, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  if (ab != 0) return fail(e, GMB_EHIP, "gmb_fitc_evaluate: the tile Cholesky of %s waited longer than its time-out for a tile (launch abandoned)", which);
  if (info != 0) {
    e->notpd = (int64_t)info - 1;
    return fail(e, GMB_ENOTPD, "gmb_fitc_evaluate: %s is not positive definite at row %lld", which, (long long)e->notpd);
  }
  return GMB_OK;
}

// the columns [first, first + count) of the training points as a point set of their own (the prepared arrays' stride stays Nr)
PointSet fitc_x_tile(const gmb_engine* e, const FitcTile& tl) {
  return PointSet{e->pts.xs + tl.first, e->pts.xl + tl.first, e->pts.cat + tl.first, tl.count, e->Nr};
}

// sum G o dk(rows, cols) / dtheta over `pad_rows` x `pad_cols` padded pairs, added to acc[0 .. FITC_DERIV_SUMS)
int fitc_deriv(gmb_engine* e, const PointSet& rows, int64_t pad_rows, const PointSet& cols, int64_t pad_cols, const double* G, int64_t ldg,
               double* acc) {
  FitcState& s = e->fitc;
  FitcDerivArgs a{};
  a.p = e->terms[0].cp;
  a.rows = rows;
  a.cols = cols;
  a.G = G;
  a.ldg = ldg;
  a.ti = (int)(pad_rows / TILE);
  a.tj = (int)(pad_cols / TILE);
  a.part = s.dredpart;
  const int64_t nblk = (int64_t)a.ti * a.tj;
  const dim3 grid((unsigned)nblk);
  ev_begin(e, e->stream, EV_FITC, 0.0, a.ti, a.tj, 0, 3);
  const bool known = with_kind_nc(a.p.kind, e->nc_pad, [&](auto kind, auto nc) {
    constexpr int K = decltype(kind)::value, NC = decltype(nc)::value;
    hipLaunchKernelGGL((fitc_deriv_kernel<K, NC>), grid, dim3(256), 0, e->stream, a);
  });
  if (!known) {
    ev_end(e);
    return fail(e, GMB_EINVAL, "unknown kernel kind %d", a.p.kind);
  }
  hipLaunchKernelGGL(fitc_fold_kernel, dim3(1), dim3(256), 0, e->stream, s.dredpart, nblk, FITC_DERIV_SUMS, 0, FITC_DERIV_SUMS, acc, 1);
  ev_end(e);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// A^T of tile `tl` into V1: the cross-covariance against Z and the solve against Lu (both passes form it; DESIGN 3.17 says why)
int fitc_tile_a(gmb_engine* e, const FitcTile& tl) {
  FitcState& s = e->fitc;
  int rc = fitc_cross_cov(e, fitc_x_tile(e, tl), tl.tpad, s.sw.V1);
  if (rc) return rc;
  return fitc_solve_lt(e, fitc_factor_u(s), s.sw.V1, tl.tpad);
}

// pass 1: Lu, lambda, B = L_B L_B^T, c, w and the NLML
int fitc_pass1(gmb_engine* e, const FitcPlan& pl, double* nlml) {
  FitcState& s = e->fitc;
  const CovParams& cp = e->terms[0].cp;
  int rc;
  if ((rc = prep_points(e, s.dZ, s.m, e->D, s.mr, s.zpts.xs, s.zpts.xl, s.zpts.cat))) return rc;
  HIP_TRY(e, hipMemsetAsync(s.dacc, 0, (size_t)FITC_ACC_DOUBLES * sizeof(double), e->stream));
  {  // Kuu = k(Z, Z) + jitter I: the training build's launch on Z, a zero border row where y would sit
    CovTileArgs a{};
    a.p = cp;
    a.p.sigma2 = 0.0;
    a.rows = a.cols = fitc_z_set(s);
    a.out = s.dKuu;
    a.ldo = s.mr;
    a.ti = (int)(s.mr / TILE);
    a.tj = (int)(s.mp / TILE);
    a.mode = COV_TRAIN;
    a.lower_only = 1;
    a.tri_grid = 1;
    a.y = s.dzero;
    if ((rc = launch_cov(e, a))) return rc;
  }
  if ((rc = fitc_factor(e, fitc_factor_u(s), "k(Z, Z) + jitter I"))) return rc;
  hipLaunchKernelGGL(fitc_init_b_kernel, dim3((unsigned)((s.mr + 255) / 256), (unsigned)s.mp), dim3(256), 0, e->stream, s.dB.p, s.mr, s.mp);
  for (int64_t t = 0; t < pl.ntile; ++t) {
    const FitcTile tl = pl.tile(t);
    if ((rc = fitc_tile_a(e, tl))) return rc;
    FitcColArgs c{};
    c.At = s.sw.V1;
    c.ldt = tl.tpad;
    c.tc = tl.count;
    c.m = (int32_t)s.m;
    c.mr = s.mr;
    c.y = e->dy + tl.first;
    c.kdiag = cp.eta2;
    c.sigma2 = cp.sigma2;
    c.lam = s.dlam + tl.first;
    c.S = s.gw.S1;
    c.part = s.dcolpart + (tl.first / FITC_COL_BLOCK) * FITC_COL_SUMS;
    ev_begin(e, e->stream, EV_FITC, 0.0, (int)(tl.tpad / TILE), (int)(s.mp / TILE), 0, 2);
    hipLaunchKernelGGL(fitc_column_kernel, dim3((unsigned)(tl.tpad / FITC_COL_BLOCK)), dim3(256), 0, e->stream, c);
    ev_end(e);
    HIP_TRY(e, hipGetLastError());
    GemmArgs g{};  // B += S S^T on the lower tiles of the bordered layout, the tiles in ascending order
    g.C = s.dB;
    g.ldc = s.mr;
    g.A = s.gw.S1;
    g.lda = s.mr;
    g.B = s.gw.S1;
    g.ldb = s.mr;
    g.mt = (int)(s.mp / TILE);
    g.nt = (int)(s.mr / TILE);
    g.k = (int)tl.tpad;
    g.alpha = 1.0;
    g.beta = 1.0;
    g.tri = 1;
    if ((rc = launch_gemm(e, e->stream, g, EV_GRAD_GEMM))) return rc;
  }
  if (s.mp > s.m)
    hipLaunchKernelGGL(fitc_fix_b_kernel, dim3((unsigned)((s.mr + 255) / 256), (unsigned)(s.mp - s.m)), dim3(256), 0, e->stream, s.dB.p, s.mr, s.m);
  HIP_TRY(e, hipGetLastError());
  if ((rc = fitc_factor(e, fitc_factor_b(s), "B = I + A Lambda^-1 A^T"))) return rc;
  // c = row m of the factored bordered matrix, c^T c; the column sums; w = L_B^-T c by blocked back substitution
  double* c = s.dcw;
  double* w = s.dcw + s.mp;
  double* rhs = s.dcw + 2 * s.mp;
  HIP_TRY(e, hipMemsetAsync(s.dcw, 0, (size_t)(3 * s.mp) * sizeof(double), e->stream));
  hipLaunchKernelGGL(extract_v_kernel, dim3(EXTRACT_V_BLOCKS), dim3(TILE), 0, e->stream, s.dB.p, s.mr, s.m, c, s.dscalB + 1);
  hipLaunchKernelGGL(fitc_fold_kernel, dim3(1), dim3(256), 0, e->stream, s.dcolpart.p, pl.col_blocks(), FITC_COL_SUMS, 0, 2, s.dacc.p, 0);
  HIP_TRY(e, hipMemcpyAsync(rhs, c, (size_t)s.m * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  const TriOperand L{s.dB, s.mr, s.dB, s.mr, (int64_t)TILE * (s.mr + 1)};
  for (int b = (int)(s.mp / TILE) - 1; b >= 0; --b) {
    hipLaunchKernelGGL(backsub_diag_kernel, dim3(1), dim3(256), 0, e->stream, L, (int64_t)b, s.m, rhs, w);
    if (b > 0) hipLaunchKernelGGL(backsub_update_kernel, dim3((unsigned)(32 * b)), dim3(256), 0, e->stream, L, (int64_t)b, s.m, w, rhs);
  }
  HIP_TRY(e, hipGetLastError());
  double hb[2] = {0.0, 0.0}, ha[2] = {0.0, 0.0};
  HIP_TRY(e, hipMemcpyAsync(hb, s.dscalB, 2 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipMemcpyAsync(ha, s.dacc, 2 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  *nlml = 0.5 * ha[0] + hb[0] + 0.5 * (ha[1] - hb[1]) + 0.5 * (double)e->N * std::log(2.0 * M_PI);
  if (!std::isfinite(*nlml)) {
    e->notpd = 0;
    return fail(e, GMB_ENOTPD, "gmb_fitc_evaluate: the factorisation produced non-finite values");
  }
  return GMB_OK;
}

// pass 2: the gradient by reverse mode, tile by tile (fitc.hpp; the formulas are DESIGN 3.17's)
int fitc_pass2(gmb_engine* e, const FitcPlan& pl, double* grad) {
  FitcState& s = e->fitc;
  const FactorRef fu = fitc_factor_u(s), fb = fitc_factor_b(s);
  const double* w = s.dcw + s.mp;
  int rc;
  HIP_TRY(e, hipMemsetAsync(s.dP, 0, (size_t)(s.mp * s.mp) * sizeof(double), e->stream));
  for (int64_t t = 0; t < pl.ntile; ++t) {
    const FitcTile tl = pl.tile(t);
    const int64_t tp = tl.tpad;
    double* V1 = s.sw.V1;
    double* V2 = s.sw.V2;
    if ((rc = fitc_tile_a(e, tl))) return rc;  // A^T
    HIP_TRY(e, hipMemcpyAsync(V2, V1, (size_t)(tp * s.mp) * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    if ((rc = fitc_solve_lt(e, fb, V2, tp))) return rc;  // C^T = A^T L_B^-T
    FitcRowArgs r{};
    r.At = V1;
    r.Ct = V2;
    r.ldt = tp;
    r.tc = tl.count;
    r.m = (int32_t)s.m;
    r.w = w;
    r.y = e->dy + tl.first;
    r.lam = s.dlam + tl.first;
    r.alpha = s.dalpha + tl.first;
    r.d = s.dd + tl.first;
    r.part = s.dcolpart + (tl.first / FITC_COL_BLOCK) * FITC_COL_SUMS;
    ev_begin(e, e->stream, EV_FITC, 0.0, (int)(tp / TILE), (int)(s.mp / TILE), 0, 2);
    hipLaunchKernelGGL(fitc_row_kernel, dim3((unsigned)(tp / FITC_COL_BLOCK)), dim3(256), 0, e->stream, r);
    ev_end(e);
    HIP_TRY(e, hipGetLastError());
    if ((rc = fitc_solve_l(e, fb, V2, tp))) return rc;  // H^T = Lambda^-1 C^T L_B^-1
    ev_begin(e, e->stream, EV_FITC, 0.0, (int)(tp / TILE), (int)(s.mp / TILE), 0, 2);
    hipLaunchKernelGGL(fitc_adjoint_kernel, dim3((unsigned)((tp + 255) / 256), (unsigned)s.mp), dim3(256), 0, e->stream, V2, V1, tp, tl.count,
                       (int32_t)s.m, r.alpha, r.d, w);
    ev_end(e);
    HIP_TRY(e, hipGetLastError());
    if ((rc = fitc_solve_l(e, fu, V2, tp))) return rc;  // G_uf^T = T^T Lu^-1
    if ((rc = fitc_deriv(e, fitc_x_tile(e, tl), tp, fitc_z_set(s), s.mp, V2, tp, s.dacc + 8))) return rc;
    // P += G_uf A^T: both blocks into the GEMM's operand layout (inducing index fastest), the tiles in ascending order
    ev_begin(e, e->stream, EV_FITC, 0.0, (int)(tp / TILE), (int)(s.mp / TILE), 0, 2);
    if ((rc = launch_transpose(e, e->stream, V1, tp, s.gw.S1, s.mr, (int)tp, (int)s.mp))) return rc;
    if ((rc = launch_transpose(e, e->stream, V2, tp, s.gw.S2, s.mr, (int)tp, (int)s.mp))) return rc;
    ev_end(e);
    GemmArgs g{};
    g.C = s.dP;
    g.ldc = s.mp;
    g.A = s.gw.S1;
    g.lda = s.mr;
    g.B = s.gw.S2;
    g.ldb = s.mr;
    g.mt = g.nt = (int)(s.mp / TILE);
    g.k = (int)tp;
    g.alpha = 1.0;
    g.beta = 1.0;
    if ((rc = launch_gemm(e, e->stream, g, EV_GRAD_GEMM))) return rc;
  }
  // G_uu = -1/2 P Lu^-1 (the factor -1/2 is the host's), reduced against dk(Z, Z)
  if ((rc = fitc_solve_l(e, fu, s.dP, s.mp))) return rc;
  if ((rc = fitc_deriv(e, fitc_z_set(s), s.mp, fitc_z_set(s), s.mp, s.dP, s.mp, s.dacc + 32))) return rc;
  hipLaunchKernelGGL(fitc_fold_kernel, dim3(1), dim3(256), 0, e->stream, s.dcolpart.p, pl.col_blocks(), FITC_COL_SUMS, 2, 1, s.dacc + 2, 0);
  HIP_TRY(e, hipGetLastError());
  double h[FITC_ACC_DOUBLES];
  HIP_TRY(e, hipMemcpyAsync(h, s.dacc, sizeof h, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  // chain rule (fitc.hpp: fitc_deriv_kernel): theta = [ls | eta | sigma]
  const gmb_kernel_spec& sp = e->spec;
  const gmb_engine::Term& tr = e->terms[0];
  const double* uf = h + 8;
  const double* uu = h + 32;
  const double sum_d = h[2], eta = tr.eta;
  const int n_ls = sp.ard ? sp.n_cont : 1;
  for (int i = 0; i < n_ls; ++i) grad[i] = 0.0;
  for (int c = 0; c < sp.n_cont; ++c) grad[sp.ard ? c : 0] += -2.0 * tr.pa.inv_ls[c] * (uf[c] - 0.5 * uu[c]);
  grad[n_ls] = (2.0 / eta) * (uf[FITC_DERIV_SUMS - 1] - 0.5 * uu[FITC_DERIV_SUMS - 1]) + eta * sum_d;
  grad[n_ls + 1] = e->theta[n_ls + 1] * sum_d;
  for (int i = 0; i < n_ls + 2; ++i)
    if (!std::isfinite(grad[i])) return fail(e, GMB_ENOTPD, "gmb_fitc_evaluate: the gradient is not finite");
  return GMB_OK;
}

int fitc_evaluate_impl(gmb_engine* e, const double* theta, int32_t n, double* nlml, double* grad) {
  const char* what = "gmb_fitc_evaluate";
  if (!e || !theta || !nlml) return GMB_EINVAL;
  FitcState& s = e->fitc;
  if (!s.have_z) return fail(e, GMB_EINVAL, "%s: gmb_fitc_set_inducing has not been called for this data and kernel", what);
  int rc = set_theta(e, theta, n, nullptr);  // (clears s.resident)
  if (rc) return rc;
  if ((rc = fitc_scope(e, what))) return rc;
  e->notpd = -1;
  FitcPlan pl;
  if ((rc = fitc_plan_for(e, what, s.m, &pl))) return rc;
  const int D = e->D;
  if ((rc = fitc_reserve(e, what, pl, [&](auto& v) { return fitc_evaluate_buffers(s, pl, D, v); }))) return rc;
  rc = fitc_pass1(e, pl, nlml);
  if (!rc) {
    s.resident = true;
    if (grad) rc = fitc_pass2(e, pl, grad);
  }
  const hipError_t sync = hipStreamSynchronize(e->stream);
  ev_collect(e);
  if (rc) return rc;
  HIP_TRY(e, sync);
  return GMB_OK;
}

int fitc_predict_impl(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise, double* mean, double* var,
                      int32_t memspace) {
  const char* what = "gmb_fitc_predict";
  if (!e) return GMB_EINVAL;
  FitcState& s = e->fitc;
  if (!s.have_z) return fail(e, GMB_EINVAL, "%s: gmb_fitc_set_inducing has not been called for this data and kernel", what);
  if (!s.resident || !e->have_theta)
    return fail(e, GMB_EINVAL, "%s: no sparse state is resident for the current theta, data and inducing points: call gmb_fitc_evaluate first", what);
  if (M < 0 || (M > 0 && (!Xs || !mean || !var)) || ldxs < e->D) return fail(e, GMB_EINVAL, "bad Xs/M/ldxs/mean/var");
  if (M == 0) return GMB_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  FitcPlan pl;
  int rc = fitc_plan_for(e, what, s.m, &pl);
  if (rc) return rc;
  const int64_t Mt = pl.predict_rows(M);
  const int D = e->D;
  if ((rc = fitc_reserve(e, what, pl, [&](auto& v) { return fitc_predict_buffers(s, pl, (double)Mt, D, v); }))) return rc;
  const CopyKinds ck = copy_kinds(memspace);
  const FactorRef fu = fitc_factor_u(s), fb = fitc_factor_b(s);
  const double* w = s.dcw + s.mp;
  auto tiles = [&]() -> int {
    for (int64_t m0 = 0; m0 < M; m0 += Mt) {
      const int64_t mc = std::min<int64_t>(Mt, M - m0);
      const int64_t mpad = round_up(mc, TILE);
      HIP_TRY(e, hipMemcpy2DAsync(s.tp.Xs, D * sizeof(double), Xs + m0 * ldxs, ldxs * sizeof(double), D * sizeof(double), mc, ck.in, e->stream));
      if ((rc = prep_points(e, s.tp.Xs, mc, D, mpad, s.tp.xs, s.tp.xl, s.tp.cat))) return rc;
      const PointSet test{s.tp.xs, s.tp.xl, s.tp.cat, mc, mpad};
      if ((rc = fitc_cross_cov(e, test, mpad, s.sw.V1))) return rc;
      KssArgs k{};
      k.p = e->terms[0].cp;
      k.pts = test;
      k.with_noise = with_noise;
      k.kss = s.tp.kss;
      hipLaunchKernelGGL(kss_kernel, dim3((unsigned)((mpad + 255) / 256)), dim3(256), 0, e->stream, k);
      if ((rc = fitc_solve_lt(e, fu, s.sw.V1, mpad))) return rc;  // As^T
      HIP_TRY(e, hipMemcpyAsync(s.sw.V2, s.sw.V1, (size_t)(mpad * s.mp) * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      if ((rc = fitc_solve_lt(e, fb, s.sw.V2, mpad))) return rc;  // C*^T
      ev_begin(e, e->stream, EV_FITC, 0.0, (int)(mpad / TILE), (int)(s.mp / TILE), 0, 3);
      hipLaunchKernelGGL(fitc_predict_kernel, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, e->stream, s.sw.V1.p, s.sw.V2.p, mpad, mc,
                         (int32_t)s.m, w, s.tp.kss.p, s.tp.mean.p, s.tp.var.p);
      ev_end(e);
      HIP_TRY(e, hipGetLastError());
      HIP_TRY(e, hipMemcpyAsync(mean + m0, s.tp.mean, mc * sizeof(double), ck.out, e->stream));
      HIP_TRY(e, hipMemcpyAsync(var + m0, s.tp.var, mc * sizeof(double), ck.out, e->stream));
    }
    return GMB_OK;
  };
  return predict_end(e, nullptr, tiles());
}

// ---- GP classification by the Laplace approximation: laplace.hpp, laplace_plan.hpp, DESIGN 3.18 ------------------------------------
// Sigma is built once per evaluation into the Laplace state's own buffer; B = I + (s s^T) o Sigma of every Newton step is written
// into the factor buffer and factored there by chol_factor, its right-hand side in the border row (the factorisation turns it into
// L^-1 rhs, as it turns y into v).  FactorState is "not factored" from set_theta on and stays so: the factor buffer holds B's
// factor, which no reader of Sigma's may see; what these calls keep valid is LaplaceState::resident.

int laplace_scope(gmb_engine* e, const char* what) {
  const gmb_kernel_spec& sp = e->spec;
  if (sp.additive) return fail(e, GMB_EINVAL, "%s: additive models are not supported by the Laplace path", what);
  if (sp.out_col >= 0 || sp.n_out > 1)
    return fail(e, GMB_EINVAL, "%s: one output only, so no output table and no heteroskedastic noise (out_col = %d, n_out = %d)", what,
                sp.out_col, sp.n_out);
  if (e->periodic != 0) return fail(e, GMB_EINVAL, "%s: periodic kernels are not supported by the Laplace path", what);
  if (e->solve_hook || e->dist_mode != 0)
    return fail(e, GMB_EINVAL, "%s is not available on distributed engines (gmb_dist_*, capacity mode)", what);
  return GMB_OK;
}

double* lap_vec(gmb_engine* e, int which) { return e->lap.dvec + (int64_t)which * e->Np; }

// a phase of the call as a trace line of its own while profiling (kind 22), around the launches' lines
struct LapPhase {
  gmb_engine* e;
  size_t at = (size_t)-1;
  LapPhase(gmb_engine* e_, int which, int iter) : e(e_) {
    if (!e->profiling) return;
    ev_begin(e, e->stream, EV_LAPLACE, 0.0, (int)(e->Np / TILE), 0, iter, which);
    at = e->evs.size() - 1;
  }
  ~LapPhase() {
    if (at != (size_t)-1) (void)hipEventRecord(e->evs[at].b, e->evs[at].s);
  }
};

// out = A v from the lower triangle of the n x n matrix A (laplace.hpp: the tiles' parts, then their sum in the plan's order)
int lap_symv(gmb_engine* e, const double* A, int64_t ld, const double* v, double* out, int iter) {
  const unsigned nt = (unsigned)(e->Np / TILE);
  LapPhase ph(e, 3, iter);
  hipLaunchKernelGGL(symv_lower_kernel, dim3(nt, nt), dim3(256), 0, e->stream, A, ld, e->N, v, e->lap.dsymv.p);
  hipLaunchKernelGGL(symv_sum_kernel, dim3(nt), dim3(LAP_TILE), 0, e->stream, e->lap.dsymv.p, (int64_t)nt, e->N, out);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// pi, W, s, g, b at `fnew`, and the folded sums in dsums
int lap_likelihood(gmb_engine* e, const double* fnew, const double* fold, const double* a, int iter) {
  LaplaceState& s = e->lap;
  LaplaceLikArgs k{};
  k.fnew = fnew, k.fold = fold, k.a = a, k.y = e->dy;
  k.n = e->N, k.np = e->Np;
  k.pi = lap_vec(e, LV_PI), k.W = lap_vec(e, LV_W), k.s = lap_vec(e, LV_S), k.g = lap_vec(e, LV_G), k.b = lap_vec(e, LV_B);
  k.part = s.dlikpart;
  const int64_t nblk = (e->Np + LAP_LIK_BLOCK - 1) / LAP_LIK_BLOCK;
  LapPhase ph(e, 4, iter);
  hipLaunchKernelGGL(laplace_lik_kernel, dim3((unsigned)nblk), dim3(LAP_LIK_BLOCK), 0, e->stream, k);
  hipLaunchKernelGGL(laplace_fold_kernel, dim3(1), dim3(256), 0, e->stream, s.dlikpart.p, nblk, s.dsums.p);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// B = I + (s s^T) o Sigma into the factor buffer with `rhs` (or 0) in the border row, its Cholesky, and L^-1 rhs into dv.  Nothing is
// synchronised: lap_factor_look reads the failure index and the abort word.
int lap_factor_enqueue(gmb_engine* e, const double* rhs, CholResult* res, int iter) {
  LaplaceState& s = e->lap;
  {
    LaplaceScaleArgs k{};
    k.src = s.dS, k.lds = e->ld, k.out = e->dA, k.ldo = e->ld;
    k.n = e->N, k.rows = e->Nr;
    k.s = lap_vec(e, LV_S), k.u = nullptr, k.rhs = rhs, k.mode = 0;
    LapPhase ph(e, 1, iter);
    hipLaunchKernelGGL(laplace_scale_kernel, dim3((unsigned)e->Np, (unsigned)((e->Nr + 255) / 256)), dim3(256), 0, e->stream, k);
    HIP_TRY(e, hipGetLastError());
  }
  LapPhase ph(e, 2, iter);
  HIP_TRY(e, hipMemsetAsync(e->dscal, 0, (size_t)SCAL_GACC_AT * sizeof(double), e->stream));
  *res = CholResult{};
  int rc = chol_factor(e, train_factor(e), CholOpts{}, res);
  if (rc) return rc;
  hipLaunchKernelGGL(extract_v_kernel, dim3(EXTRACT_V_BLOCKS), dim3(TILE), 0, e->stream, e->dA, e->ld, e->N, e->dv, e->dscal + 1);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// out = L^-T v by blocked back substitution against B's factor (`run`: the running right-hand side, Np doubles)
int lap_backsub(gmb_engine* e, const double* v, double* run, double* out, int iter) {
  LapPhase ph(e, 2, iter);
  HIP_TRY(e, hipMemsetAsync(out, 0, (size_t)e->Np * sizeof(double), e->stream));
  HIP_TRY(e, hipMemsetAsync(run, 0, (size_t)e->Np * sizeof(double), e->stream));
  HIP_TRY(e, hipMemcpyAsync(run, v, (size_t)e->N * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  const TriOperand L{e->dA, e->ld, e->dA, e->ld, (int64_t)TILE * (e->ld + 1)};
  for (int b = (int)(e->Np / TILE) - 1; b >= 0; --b) {
    hipLaunchKernelGGL(backsub_diag_kernel, dim3(1), dim3(256), 0, e->stream, L, (int64_t)b, e->N, run, out);
    if (b > 0) hipLaunchKernelGGL(backsub_update_kernel, dim3((unsigned)(32 * b)), dim3(256), 0, e->stream, L, (int64_t)b, e->N, out, run);
  }
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// the host's look at what has been enqueued: the folded sums, and (`res` given) the last factorisation's failure index, abort word
// and log-determinant
int lap_look(gmb_engine* e, const char* what, double* sums, const CholResult* res, double* logdet) {
  int32_t info = 0;
  uint32_t ab = 0;
  double ld = 0.0;
  if (sums) HIP_TRY(e, hipMemcpyAsync(sums, e->lap.dsums, LAP_LIK_SUMS * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (res) {
    HIP_TRY(e, hipMemcpyAsync(&info, e->dinfo, sizeof info, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipMemcpyAsync(&ld, e->dscal, sizeof ld, hipMemcpyDeviceToHost, e->stream));
    if (res->tiles) HIP_TRY(e, hipMemcpyAsync(&ab, e->dct + 1, sizeof ab, hipMemcpyDeviceToHost, e->stream));
  }
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  if (ab != 0) return fail(e, GMB_EHIP, "%s: the tile Cholesky of B waited longer than its time-out for a tile (launch abandoned)", what);
  if (info != 0) {
    e->notpd = (int64_t)info - 1;
    return fail(e, GMB_ENOTPD, "%s: B = I + sqrt(W) Sigma sqrt(W) is not positive definite at row %lld", what, (long long)e->notpd);
  }
  if (logdet) *logdet = ld;
  return GMB_OK;
}

int laplace_mode_and_objective(gmb_engine* e, const char* what, double* nlq) {
  LaplaceState& s = e->lap;
  const int64_t Np = e->Np;
  const unsigned vgrid = (unsigned)((Np + 255) / 256);
  int rc;
  {
    LapPhase ph(e, 0, 0);
    if ((rc = build_sigma(e, s.dS, e->ld))) return rc;
  }
  // a = f = 0 in every evaluation: the result does not depend on what was evaluated before
  HIP_TRY(e, hipMemsetAsync(s.dvec, 0, (size_t)(LAP_VECTORS * Np) * sizeof(double), e->stream));
  double* f = lap_vec(e, LV_F0);
  double* fc = lap_vec(e, LV_F1);
  double* a = lap_vec(e, LV_A);
  double* ac = lap_vec(e, LV_AC);
  double* ah = lap_vec(e, LV_AH);
  double *t1 = lap_vec(e, LV_T1), *t2 = lap_vec(e, LV_T2), *t3 = lap_vec(e, LV_T3);
  double sums[LAP_LIK_SUMS];
  s.iterations = s.halvings = 0;
  s.step = 0.0;
  if ((rc = lap_likelihood(e, f, f, a, 0))) return rc;
  if ((rc = lap_look(e, what, sums, nullptr, nullptr))) return rc;
  if (sums[4] != 0.0)
    return fail(e, GMB_EINVAL, "%s: the labels (gmb_set_data / gmb_set_y) must be exactly 0 or 1; %.0f of %lld are not", what, sums[4], (long long)e->N);
  double psi = sums[0] - 0.5 * sums[1];
  s.psi = psi;
  bool converged = false;
  for (int it = 1; it <= s.max_iter && !converged; ++it) {
    // a^ = b - s o B^-1 (s o (Sigma b))
    if ((rc = lap_symv(e, s.dS, e->ld, lap_vec(e, LV_B), t1, it))) return rc;
    hipLaunchKernelGGL(laplace_mul_kernel, dim3(vgrid), dim3(256), 0, e->stream, lap_vec(e, LV_S), t1, e->N, Np, t2);
    CholResult res;
    if ((rc = lap_factor_enqueue(e, t2, &res, it))) return rc;
    if ((rc = lap_backsub(e, e->dv, t1, t3, it))) return rc;
    hipLaunchKernelGGL(laplace_ahat_kernel, dim3(vgrid), dim3(256), 0, e->stream, lap_vec(e, LV_B), lap_vec(e, LV_S), t3, a, 1.0, e->N, Np, ah, ac);
    HIP_TRY(e, hipGetLastError());
    // the step: t = 1, halved while Psi falls
    double t = 1.0, psi_c = psi;
    bool accepted = false;
    for (int h = 0; h <= 20; ++h) {
      if (h > 0) hipLaunchKernelGGL(laplace_step_kernel, dim3(vgrid), dim3(256), 0, e->stream, a, ah, t, e->N, Np, ac);
      if ((rc = lap_symv(e, s.dS, e->ld, ac, fc, it))) return rc;
      if ((rc = lap_likelihood(e, fc, f, ac, it))) return rc;
      if ((rc = lap_look(e, what, sums, h == 0 ? &res : nullptr, nullptr))) return rc;
      psi_c = sums[0] - 0.5 * sums[1];
      if (sums[5] != 0.0 || !std::isfinite(psi_c)) {
        e->notpd = 0;
        return fail(e, GMB_ENOTPD, "%s: the Newton step of iteration %d produced non-finite values", what, it);
      }
      if (psi_c >= psi - 1e-14 * std::fabs(psi)) {
        accepted = true;
        break;
      }
      t *= 0.5;
      if (h < 20) ++s.halvings;
    }
    s.iterations = it;
    if (!accepted)
      return fail(e, GMB_ENOCONV, "%s: Psi still falls after 20 halvings of the step of iteration %d (Psi = %.17g)", what, it, psi);
    std::swap(f, fc);
    std::swap(a, ac);
    psi = psi_c;
    s.psi = psi;
    s.step = sums[2];
    converged = sums[2] <= s.tol * std::max(1.0, sums[3]);
  }
  // the vectors the mode ended in: `a` may be either of the two (the readers ask lap_mode_vectors)
  s.f_swapped = f != lap_vec(e, LV_F0);
  if (!converged)
    return fail(e, GMB_ENOCONV, "%s: no convergence in %d Newton iterations (last step %.3g, tol %.3g)", what, s.max_iter, s.step, s.tol);
  // W at the mode itself: B's factor for the log-determinant, the gradient and the predictions
  CholResult res;
  if ((rc = lap_factor_enqueue(e, nullptr, &res, s.iterations + 1))) return rc;
  double logdet = 0.0;
  if ((rc = lap_look(e, what, nullptr, &res, &logdet))) return rc;
  *nlq = -psi + logdet;
  if (!std::isfinite(*nlq)) {
    e->notpd = 0;
    return fail(e, GMB_ENOTPD, "%s: the factorisation produced non-finite values", what);
  }
  return GMB_OK;
}

// where the mode lies: the two f vectors and the two a vectors change roles with every accepted step, together
void lap_mode_vectors(gmb_engine* e, double** f, double** a) {
  *f = lap_vec(e, e->lap.f_swapped ? LV_F1 : LV_F0);
  *a = lap_vec(e, e->lap.f_swapped ? LV_AC : LV_A);
}

// Alg. 5.1 folded into the exact path's trace pass: Z' = R + u u^T in the inverse's buffer, a' = a^ + u in the gradient's alpha
int laplace_gradient(gmb_engine* e, double* grad) {
  LaplaceState& s = e->lap;
  const int64_t Np = e->Np;
  const unsigned vgrid = (unsigned)((Np + 255) / 256);
  const int it = s.iterations + 1;
  int rc;
  double *f, *a;
  lap_mode_vectors(e, &f, &a);
  double *t1 = lap_vec(e, LV_T1), *t2 = lap_vec(e, LV_T2), *t3 = lap_vec(e, LV_T3), *s2 = lap_vec(e, LV_S2), *u = lap_vec(e, LV_U);
  {
    LapPhase ph(e, 5, it);
    if ((rc = tri_inverse_pair(e, false))) return rc;
    if ((rc = inverse_from_pair(e))) return rc;  // B^-1, lower triangle of dW; L is back in the factor buffer
  }
  hipLaunchKernelGGL(laplace_s2_kernel, dim3(vgrid), dim3(256), 0, e->stream, e->dW.p, Np, lap_vec(e, LV_PI), e->N, Np, s2);
  if ((rc = lap_symv(e, s.dS, e->ld, s2, t1, it))) return rc;
  hipLaunchKernelGGL(laplace_mul_kernel, dim3(vgrid), dim3(256), 0, e->stream, lap_vec(e, LV_S), t1, e->N, Np, t2);
  if ((rc = lap_symv(e, e->dW, Np, t2, t3, it))) return rc;
  hipLaunchKernelGGL(laplace_u_kernel, dim3(vgrid), dim3(256), 0, e->stream, s2, lap_vec(e, LV_S), t3, a, e->N, Np, u, e->dalpha.p);
  {
    LaplaceScaleArgs k{};
    k.src = nullptr, k.lds = 0, k.out = e->dW, k.ldo = Np;
    k.n = e->N, k.rows = Np;
    k.s = lap_vec(e, LV_S), k.u = u, k.rhs = nullptr, k.mode = 1;
    LapPhase ph(e, 1, it);
    hipLaunchKernelGGL(laplace_scale_kernel, dim3((unsigned)Np, (unsigned)((Np + 255) / 256)), dim3(256), 0, e->stream, k);
    HIP_TRY(e, hipGetLastError());
  }
  std::vector<double> h;
  {
    LapPhase ph(e, 6, it);
    if ((rc = grad_reduce(e, 0, 1, e->dW, Np, false, h, GradLanding{}))) return rc;
  }
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  if ((rc = grad_chain_rule(e, h, grad))) return rc;
  for (size_t i = 0; i < e->theta.size(); ++i)
    if (!std::isfinite(grad[i])) return fail(e, GMB_ENOTPD, "gmb_laplace_evaluate: the gradient is not finite");
  return GMB_OK;
}

int laplace_evaluate_impl(gmb_engine* e, const double* theta, int32_t n, double* nlq, double* grad) {
  const char* what = "gmb_laplace_evaluate";
  if (!e || !theta || !nlq) return GMB_EINVAL;
  if (!e->have_spec) return fail(e, GMB_EINVAL, "gmb_set_kernel must precede %s", what);
  if (e->N <= 0) return fail(e, GMB_EINVAL, "gmb_set_data must precede %s", what);
  int rc = laplace_scope(e, what);
  if (rc) return rc;
  LaplaceState& s = e->lap;
  if ((rc = set_theta(e, theta, n, nullptr))) return rc;  // (FactorState: not factored, whatever was there; the Laplace state dropped)
  s.dropped_by = "the last gmb_laplace_evaluate failed";
  e->notpd = -1;
  LaplacePlan pl;
  if (pl.make(e->N)) return fail(e, GMB_EINVAL, "%s: N = %lld is out of range (at most %lld)", what, (long long)e->N, (long long)LAP_MAX_N);
  {
    auto list = [&](auto& v) {
      return laplace_evaluate_buffers(s, pl, v) && v.buf(e->dA, (double)e->ld * (double)e->Np) &&
             (!grad || (v.buf(e->dW, (double)e->Np * (double)e->Np) && v.buf(e->dalpha, 3.0 * (double)e->Np)));
    };
    Budget need;
    list(need);
    double free_b;
    if ((rc = device_free_bytes(e, &free_b))) return rc;
    if (need.fresh > free_b)
      return fail(e, GMB_ENOMEM, "%s: N = %lld needs %.0f bytes on the device (Sigma, the factor buffer%s: %.0f each), %.0f more than the engine "
                                 "holds now; %.0f bytes are free -- nothing was computed",
                  what, (long long)e->N, need.total, grad ? " and the inverse's" : "", 8.0 * pl.sigma_doubles(), need.fresh, free_b);
    Reserver take{e->pool};
    list(take);
    if (take.rc) return take.rc;
  }
  rc = laplace_mode_and_objective(e, what, nlq);
  if (!rc && grad) rc = laplace_gradient(e, grad);
  const hipError_t sync = hipStreamSynchronize(e->stream);
  ev_collect(e);
  if (rc) return rc;
  HIP_TRY(e, sync);
  s.resident = true;
  return GMB_OK;
}

int laplace_require_resident(gmb_engine* e, const char* what) {
  if (!e) return GMB_EINVAL;
  if (!e->lap.resident || !e->have_theta)
    return fail(e, GMB_EINVAL, "%s: no Laplace state is resident for the current data, labels, kernel and theta: %s -- call gmb_laplace_evaluate first",
                what, e->lap.dropped_by);
  return GMB_OK;
}

// Alg. 3.2 on the prediction's own pieces: the cross-covariance launch, the mean k*^T g by the reduction a product-form prediction
// takes its mean with, the columns scaled by s, the strip solve against B's factor, the variance reduction
int laplace_predict_impl(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, double* mean, double* var, int32_t memspace) {
  const char* what = "gmb_laplace_predict";
  int rc = laplace_require_resident(e, what);
  if (rc) return rc;
  if (M < 0 || (M > 0 && (!Xs || !mean || !var)) || ldxs < e->D) return fail(e, GMB_EINVAL, "bad Xs/M/ldxs/mean/var");
  if (M == 0) return GMB_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  reset_predict_timings(e);
  const int64_t Mt = predict_tile_rows(e, M);
  if ((rc = predict_workspace(e, Mt))) return rc;
  const int nchunk = red_chunks(e->N);
  e->tm.predict_gemm_form = 0;
  const CopyKinds ck = copy_kinds(memspace);
  PhaseTimer tp(e);
  auto tiles = [&]() -> int {
    for (int64_t m0 = 0; m0 < M; m0 += Mt) {
      const int64_t mc = std::min<int64_t>(Mt, M - m0);
      const int64_t mpad = round_up(mc, TILE);
      if ((rc = predict_cross_cov(e, 1u, Xs + m0 * ldxs, mc, mpad, ldxs, 0, ck.in))) return rc;
      const unsigned mblocks = (unsigned)(mpad / 256 + (mpad % 256 ? 1 : 0));
      hipLaunchKernelGGL(predict_mean_partial_kernel, dim3(mblocks, nchunk), dim3(256), 0, e->stream, e->pw.dV, mpad, lap_vec(e, LV_G), e->N, e->dpart,
                         mpad);
      hipLaunchKernelGGL(predict_mean_final_kernel, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, e->stream, e->dpart, nchunk, mpad, mc,
                         e->pw.dmean);
      HIP_TRY(e, hipMemcpyAsync(mean + m0, e->pw.dmean, mc * sizeof(double), ck.out, e->stream));
      hipLaunchKernelGGL(laplace_colscale_kernel, dim3(mblocks, (unsigned)((e->N + LAP_SCALE_COLS - 1) / LAP_SCALE_COLS)), dim3(256), 0, e->stream,
                         e->pw.dV.p, mpad, e->N, lap_vec(e, LV_S));
      HIP_TRY(e, hipGetLastError());
      if ((rc = predict_solve_v(e, mpad, false))) return rc;
      if ((rc = predict_reduce(e, mc, mpad, false))) return rc;  // (its mean, against the border row's v, is not the latent mean)
      HIP_TRY(e, hipMemcpyAsync(var + m0, e->pw.dvar, mc * sizeof(double), ck.out, e->stream));
    }
    return GMB_OK;
  };
  return predict_end(e, &tp, tiles());
}

}  // namespace

extern "C" {

int gmb_fitc_set_inducing(gmb_engine* e, const double* Z, int64_t m, int64_t ldz, int32_t memspace) {
  return fitc_set_inducing_impl(e, Z, m, ldz, memspace);
}

int gmb_fitc_evaluate(gmb_engine* e, const double* theta, int32_t n, double* nlml, double* grad) {
  return fitc_evaluate_impl(e, theta, n, nlml, grad);
}

int gmb_fitc_predict(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise, double* mean, double* var,
                     int32_t memspace) {
  return fitc_predict_impl(e, Xs, M, ldxs, with_noise, mean, var, memspace);
}

int64_t gmb_debug_fitc_plan(int64_t N, int64_t m, int64_t* out, int64_t cap) {
  FitcPlan pl;
  const int bad = pl.make(N, m);
  if (bad) return -(int64_t)bad;
  FitcState st;  // (nothing allocated: a Budget only reads what the buffers hold)
  Budget fixed, blocks, columns;
  fitc_fixed_buffers(st, pl, 1, fixed);
  fitc_block_buffers(st, pl, (double)pl.tmax, true, blocks);
  fitc_column_buffers(st, pl, columns);
  return fitc_plan_dump(pl, fixed.total, blocks.total, columns.total, out, cap);
}

int gmb_laplace_evaluate(gmb_engine* e, const double* theta, int32_t n, double* nlq, double* grad) {
  return laplace_evaluate_impl(e, theta, n, nlq, grad);
}

int gmb_laplace_predict(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, double* mean, double* var, int32_t memspace) {
  return laplace_predict_impl(e, Xs, M, ldxs, mean, var, memspace);
}

int gmb_laplace_info(const gmb_engine* e, gmb_laplace_stats* out) {
  if (!e || !out) return GMB_EINVAL;
  out->iterations = e->lap.iterations;
  out->halvings = e->lap.halvings;
  out->psi = e->lap.psi;
  out->step = e->lap.step;
  return GMB_OK;
}

int gmb_laplace_copy_mode(const gmb_engine* ce, double* f, double* a) {
  gmb_engine* e = const_cast<gmb_engine*>(ce);
  int rc = laplace_require_resident(e, "gmb_laplace_copy_mode");
  if (rc) return rc;
  HIP_TRY(e, hipSetDevice(e->device));
  double *df, *da;
  lap_mode_vectors(e, &df, &da);
  if (f) HIP_TRY(e, hipMemcpy(f, df, (size_t)e->Np * sizeof(double), hipMemcpyDeviceToHost));
  if (a) HIP_TRY(e, hipMemcpy(a, da, (size_t)e->Np * sizeof(double), hipMemcpyDeviceToHost));
  return GMB_OK;
}

int gmb_laplace_set_options(gmb_engine* e, double tol, int32_t max_iter) {
  if (!e) return GMB_EINVAL;
  if (!(tol > 0.0) || !std::isfinite(tol)) return fail(e, GMB_EINVAL, "gmb_laplace_set_options: tol must be a positive number");
  if (max_iter < 1 || max_iter > 40) return fail(e, GMB_EINVAL, "gmb_laplace_set_options: max_iter = %d (1 .. 40)", max_iter);
  e->lap.tol = tol;
  e->lap.max_iter = max_iter;
  return GMB_OK;
}

int64_t gmb_debug_laplace_plan(int64_t N, int64_t* out, int64_t cap) {
  LaplacePlan pl;
  const int bad = pl.make(N);
  if (bad) return -(int64_t)bad;
  LaplaceState st;  // (nothing allocated: a Budget only reads what the buffers hold)
  Budget need;
  laplace_evaluate_buffers(st, pl, need);
  return laplace_plan_dump(pl, need.total, out, cap);
}

int gmb_debug_laplace_symv(gmb_engine* e, const double* v, double* out) {
  int rc = laplace_require_resident(e, "gmb_debug_laplace_symv");
  if (rc) return rc;
  if (!v || !out) return fail(e, GMB_EINVAL, "gmb_debug_laplace_symv: null v / out");
  HIP_TRY(e, hipSetDevice(e->device));
  double *t1 = lap_vec(e, LV_T1), *t2 = lap_vec(e, LV_T2);
  HIP_TRY(e, hipMemcpyAsync(t1, v, (size_t)e->Np * sizeof(double), hipMemcpyHostToDevice, e->stream));
  if ((rc = lap_symv(e, e->lap.dS, e->ld, t1, t2, 0))) return rc;
  HIP_TRY(e, hipMemcpyAsync(out, t2, (size_t)e->Np * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  ev_collect(e);
  return GMB_OK;
}

int gmb_nlml(gmb_engine* e, double* nlml, double* grad) {
  int rc = require_ready(e, true);
  if (rc) return rc;
  if (!nlml) return fail(e, GMB_EINVAL, "nlml output pointer is null");
  *nlml = 0.5 * (double)e->N * std::log(2.0 * M_PI) + e->logdet + 0.5 * e->vnorm2;
  if (grad) {
    if ((rc = require_full_factor(e, "gmb_nlml with a gradient"))) return rc;
    std::vector<double> h;
    if ((rc = grad_accumulate(e, h, nullptr))) return rc;
    return grad_chain_rule(e, h, grad);
  }
  return GMB_OK;
}

int gmb_predict(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise,
                double* mean, double* var, int32_t memspace) {
  return predict_sel(e, nullptr, "gmb_predict", Xs, M, ldxs, with_noise, mean, var, memspace);
}

int gmb_predict_terms(gmb_engine* e, uint32_t terms, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise,
                      double* mean, double* var, int32_t memspace) {
  return predict_sel(e, &terms, "gmb_predict_terms", Xs, M, ldxs, with_noise, mean, var, memspace);
}

int gmb_predict_grad(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, double* grad, int64_t ldg, int32_t memspace) {
  return predict_grad_sel(e, nullptr, "gmb_predict_grad", Xs, M, ldxs, grad, ldg, memspace);
}

int gmb_predict_grad_terms(gmb_engine* e, uint32_t terms, const double* Xs, int64_t M, int64_t ldxs, double* grad, int64_t ldg,
                           int32_t memspace) {
  return predict_grad_sel(e, &terms, "gmb_predict_grad_terms", Xs, M, ldxs, grad, ldg, memspace);
}

int gmb_predict_with_grad(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise, double* mean, double* var,
                          double* dmean, double* dvar, int64_t ldg, int32_t memspace) {
  int rc = joint_ready(e, "gmb_predict_with_grad");
  if (rc) return rc;
  if (M < 0 || (M > 0 && (!Xs || !mean || !var || !dmean || !dvar)) || ldxs < e->D || ldg < e->D)
    return fail(e, GMB_EINVAL, "bad Xs/M/ldxs/mean/var/dmean/dvar/ldg");
  if (M == 0) return GMB_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  reset_predict_timings(e);
  e->tm.predict_gemm_form = 0;  // V is always solved for: W = V L^-1 follows in place, and neither dW nor U is touched
  const int64_t Mt = predict_tile_rows(e, M);
  if ((rc = predict_workspace(e, Mt))) return rc;
  if ((rc = predict_grad_workspace(e, Mt, 2))) return rc;
  const double* alpha = nullptr;
  if ((rc = resident_alpha(e, &alpha))) return predict_end(e, nullptr, rc);
  const CopyKinds ck = copy_kinds(memspace);
  const size_t row = e->D * sizeof(double);
  PhaseTimer tp(e);
  auto tiles = [&]() -> int {
    for (int64_t m0 = 0; m0 < M; m0 += Mt) {
      const int64_t mc = std::min<int64_t>(Mt, M - m0);
      const int64_t mpad = round_up(mc, TILE);
      if ((rc = predict_cross_cov(e, ALL_TERMS, Xs + m0 * ldxs, mc, mpad, ldxs, with_noise, ck.in))) return rc;
      if ((rc = predict_solve_v(e, mpad, false))) return rc;
      if ((rc = predict_reduce(e, mc, mpad, false))) return rc;
      if ((rc = predict_solve_w(e, mpad))) return rc;
      // (the tile's raw points are in dXs: predict_cross_cov; W = K(X*, X) Sigma^-1 in dV)
      if ((rc = predict_grad_tile(e, ALL_TERMS, e->pw.dXs, mc, mpad, alpha, e->pw.dV))) return rc;
      if (hipMemcpyAsync(mean + m0, e->pw.dmean, mc * sizeof(double), ck.out, e->stream) != hipSuccess ||
          hipMemcpyAsync(var + m0, e->pw.dvar, mc * sizeof(double), ck.out, e->stream) != hipSuccess ||
          hipMemcpy2DAsync(dmean + m0 * ldg, ldg * sizeof(double), e->pg.grad, row, row, mc, ck.out, e->stream) != hipSuccess ||
          hipMemcpy2DAsync(dvar + m0 * ldg, ldg * sizeof(double), e->vg_grad, row, row, mc, ck.out, e->stream) != hipSuccess)
        return fail(e, GMB_EHIP, "gmb_predict_with_grad: copying the results out failed");
    }
    return GMB_OK;
  };
  return predict_end(e, &tp, tiles());
}

// ---- joint posteriors of many small batches (predict_batches.hpp) ------------------------------------------------------------------

// Q = V V^T per batch of one tile into the covariance blocks: bw.cov = diag(k**) - Q + jitter I (V in dV, k** in dkss)
int batch_gram(gmb_engine* e, const BatchPlan& pl, const BatchTile& tl, double jitter) {
  BatchGramArgs a{};
  a.V = e->pw.dV;
  a.mpad = tl.mpad;
  a.N = e->N;
  a.nb = tl.nb;
  a.chunk = tl.chunk;
  a.q = pl.q;
  a.part = e->bw.part;
  ev_begin(e, e->stream, EV_BATCH, 2.0 * 256.0 * (double)e->N * (double)tl.nb, (int)tl.nb, (int)tl.nchunk, pl.q, 0);
  hipLaunchKernelGGL(batch_gram_partial_kernel, dim3((unsigned)tl.nb, (unsigned)tl.nchunk), dim3(64), 0, e->stream, a);
  BatchCovFinishArgs f{};
  f.part = e->bw.part;
  f.nchunk = (int32_t)tl.nchunk;
  f.q = pl.q;
  f.nb = tl.nb;
  f.kss = e->pw.dkss;
  f.jitter = jitter;
  f.cov = e->bw.cov;
  hipLaunchKernelGGL(batch_cov_finish_kernel, dim3((unsigned)((tl.mc * pl.q + 255) / 256)), dim3(256), 0, e->stream, f);
  ev_end(e);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// The walk over the terms of one tile: the prior covariance of the within-batch pairs into bw.cov and, with W = V L^-1 in dV
// (`grad`), every term's derivative sums into bw.dcov.  The tile's points are prepared per term into the prediction workspace,
// whose prepared points have served the cross-covariance.
int batch_terms(gmb_engine* e, const BatchPlan& pl, const BatchTile& tl, bool grad) {
  int rc;
  const unsigned nthreads = (unsigned)((tl.mc * pl.q + 255) / 256);  // one thread per (batch, j, l)
  if (grad) HIP_TRY(e, hipMemsetAsync(e->bw.dcov, 0, (size_t)(tl.mc * pl.q * e->D) * sizeof(double), e->stream));
  return walk_terms(e, ALL_TERMS, [&](int t) -> int {
    const gmb_engine::Term& tr = e->terms[t];
    if ((rc = prep_points(e, e->pw.dXs, tl.mc, e->D, tl.mpad, e->pw.txs, e->pw.txl, e->pw.tcat, &tr.pa))) return rc;
    BatchTermArgs ta{};
    ta.p = tr.cp;
    ta.txs = e->pw.txs;
    ta.txl = e->pw.txl;
    ta.tcat = e->pw.tcat;
    ta.mpad = tl.mpad;
    ta.nb = tl.nb;
    ta.q = pl.q;
    ta.nc_pad = e->nc_pad;
    BatchGradArgs ga{};
    BatchGradFinishArgs f{};
    if (grad) {
      ga.p = tr.cp;
      ga.test = PointSet{e->pw.txs, e->pw.txl, e->pw.tcat, tl.mc, tl.mpad};
      ga.train = train_set(e);
      ga.W = e->pw.dV;
      ga.nb = tl.nb;
      ga.chunk = tl.chunk;
      ga.q = pl.q;
      ga.part = e->bw.part;
      f.t = ta;
      f.part = e->bw.part;
      f.nchunk = (int32_t)tl.nchunk;
      f.nc = tr.pa.nc;
      f.periodic = tr.pa.periodic;
      f.D = e->D;
      for (int k = 0; k < tr.pa.nc; ++k) f.idx_cont[k] = tr.pa.idx_cont[k];
      if (tr.pa.periodic) {
        for (int d = 0; 2 * d < tr.pa.nc; ++d) f.scale[d] = 2.0 * M_PI * tr.pa.two_over_T[d];  // 2 * (2 pi / T_d)
      } else {
        for (int k = 0; k < tr.pa.nc; ++k) f.scale[k] = 2.0 * tr.pa.inv_ls[k];
      }
      for (int l = 0; l < tr.cp.n_lin; ++l) f.idx_lin[l] = tr.pa.idx_lin[l];
      f.dcov = e->bw.dcov;
    }
    const bool gen = tr.cp.n_lin > 0 || tr.cp.n_tab > 0;
    const dim3 grid((unsigned)tl.nb, (unsigned)tl.nchunk);
    const bool known = with_kind_nc(tr.cp.kind, e->nc_pad, [&](auto kind, auto nc) {
      constexpr int K = decltype(kind)::value, NC = decltype(nc)::value;
      hipLaunchKernelGGL(batch_prior_kernel<K>, dim3(nthreads), dim3(256), 0, e->stream, ta, (double*)e->bw.cov);
      if (!grad) return;
      ev_begin(e, e->stream, EV_BATCH, 2.0 * 256.0 * (double)e->N * (double)tl.nb * (NC + tr.cp.n_lin), (int)tl.nb, (int)tl.nchunk, pl.q, 1);
      if (gen) hipLaunchKernelGGL((batch_grad_partial_kernel<K, NC, true>), grid, dim3(64), 0, e->stream, ga);
      else hipLaunchKernelGGL((batch_grad_partial_kernel<K, NC, false>), grid, dim3(64), 0, e->stream, ga);
      hipLaunchKernelGGL(batch_grad_finish_kernel<K>, dim3(nthreads), dim3(256), 0, e->stream, f);
      ev_end(e);
    });
    if (!known) return fail(e, GMB_EINVAL, "unknown kernel kind %d", tr.cp.kind);
    HIP_TRY(e, hipGetLastError());
    return GMB_OK;
  });
}

int gmb_predict_batches(gmb_engine* e, const double* Xs, int64_t B, int32_t q, int64_t ldxs, double jitter, double* mean, double* cov,
                        double* dmean, int64_t ldg, double* dcov, int32_t memspace) {
  const char* what = "gmb_predict_batches";
  int rc = joint_ready(e, what);
  if (rc) return rc;
  const bool grad = dmean || dcov;
  if (q < 1 || q > BATCH_MAX_Q || B < 0)
    return fail(e, GMB_EINVAL, "%s: B = %lld batches of q = %d points (B >= 0 and 1 <= q <= %d are required)", what, (long long)B, (int)q,
                BATCH_MAX_Q);
  if ((B > 0 && (!Xs || !mean || !cov)) || (dmean == nullptr) != (dcov == nullptr) || ldxs < e->D || (grad && ldg < e->D) || !(jitter >= 0.0))
    return fail(e, GMB_EINVAL, "%s: bad Xs/ldxs/jitter/mean/cov/ldg, or one of dmean and dcov without the other", what);
  if (B == 0) return GMB_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  // the plan first (host arithmetic), then the bytes against the device, then the allocation: a refusal has touched nothing
  BatchPlan pl;
  if (pl.make(e->N, e->Np, B, q))
    return fail(e, GMB_EINVAL, "%s: B = %lld batches of q = %d points are more than a call takes (B q <= 2^40)", what, (long long)B, (int)q);
  int nacc = 1;  // accumulators per (chunk, batch): Q alone, or a term's prepared columns and linear sums
  if (grad)
    for (const gmb_engine::Term& tr : e->terms) nacc = std::max<int>(nacc, e->nc_pad + tr.cp.n_lin);
  const double pg_part = ((double)PG_TARGET_WGS * PG_PTS + (double)pl.mt) * (e->nc_pad + MAX_LIN);  // (predict_grad_workspace, one set)
  {
    Budget need;
    batch_buffers(*e, pl, nacc, grad, pg_part, need);
    double free_b;
    if ((rc = device_free_bytes(e, &free_b))) return rc;
    if (need.fresh > free_b)
      return fail(e, GMB_ENOMEM, "%s: B = %lld batches of q = %d points behind N = %lld need %.0f bytes on the device (V of one M-tile: %.0f), "
                                 "%.0f more than it holds for the engine now; %.0f bytes are free -- nothing was computed",
                  what, (long long)B, (int)q, (long long)e->N, need.total, 8.0 * (double)pl.mt * (double)e->Np, need.fresh, free_b);
    Reserver take{e->pool};
    batch_buffers(*e, pl, nacc, grad, pg_part, take);
    if (take.rc) return take.rc;
  }
  reset_predict_timings(e);
  e->tm.predict_gemm_form = 0;  // V is always solved for, as in gmb_predict_with_grad: neither dW nor U is touched
  const double* alpha = nullptr;
  if (grad && (rc = resident_alpha(e, &alpha))) return predict_end(e, nullptr, rc);
  const CopyKinds ck = copy_kinds(memspace);
  const size_t row = e->D * sizeof(double);
  const int64_t qq = (int64_t)q * q;
  PhaseTimer tp(e);
  auto tiles = [&]() -> int {
    for (int64_t t = 0; t < pl.ntile; ++t) {
      const BatchTile tl = pl.tile(t);
      const int64_t m0 = tl.first * q;
      if ((rc = predict_cross_cov(e, ALL_TERMS, Xs + m0 * ldxs, tl.mc, tl.mpad, ldxs, 0, ck.in))) return rc;
      if ((rc = predict_solve_v(e, tl.mpad, false))) return rc;
      if ((rc = predict_reduce(e, tl.mc, tl.mpad, false))) return rc;
      if ((rc = batch_gram(e, pl, tl, jitter))) return rc;
      if (grad) {
        if ((rc = predict_solve_w(e, tl.mpad))) return rc;
        // (the tile's raw points are in dXs: predict_cross_cov; W = K(X*, X) Sigma^-1 in dV)
        if ((rc = predict_grad_tile(e, ALL_TERMS, e->pw.dXs, tl.mc, tl.mpad, alpha, nullptr))) return rc;
      }
      if ((rc = batch_terms(e, pl, tl, grad))) return rc;
      if (hipMemcpyAsync(mean + m0, e->pw.dmean, tl.mc * sizeof(double), ck.out, e->stream) != hipSuccess ||
          hipMemcpyAsync(cov + tl.first * qq, e->bw.cov, tl.nb * qq * sizeof(double), ck.out, e->stream) != hipSuccess)
        return fail(e, GMB_EHIP, "%s: copying the values out failed", what);
      if (grad && (hipMemcpy2DAsync(dmean + m0 * ldg, ldg * sizeof(double), e->pg.grad, row, row, tl.mc, ck.out, e->stream) != hipSuccess ||
                   hipMemcpyAsync(dcov + tl.first * qq * e->D, e->bw.dcov, tl.nb * qq * row, ck.out, e->stream) != hipSuccess))
        return fail(e, GMB_EHIP, "%s: copying the gradients out failed", what);
    }
    return GMB_OK;
  };
  return predict_end(e, &tp, tiles());
}

int64_t gmb_debug_batch_plan(int64_t N, int64_t Np, int64_t B, int32_t q, int64_t* out, int64_t cap) { return batch_plan_dump(N, Np, B, q, out, cap); }

// ---- pathwise posterior draws (pathwise.hpp, paths_plan.hpp) ------------------------------------------------------------------------

namespace {

// the all-draws kernel over one tile of prepared points (txs: stride tpad) into paths.out ([draw of Sp][point of tl.mpad]); with
// `train` the contraction runs over the training points and the features (pl.N = e->N), without over the features alone (pl.N = 0)
int paths_eval_tile(gmb_engine* e, const PathsPlan& pl, const PathsTile& tl, const double* txs, int64_t tpad, bool train) {
  PathState& st = e->paths;
  const gmb_engine::Term& tr = e->terms[0];
  PathsEvalArgs a{};
  a.txs = txs;
  a.tpad = tpad;
  a.mc = tl.mc;
  a.xs = e->pts.xs;
  a.npad = e->Nr;
  a.N = train ? e->N : 0;
  a.A = st.A;
  a.wt = st.wt;
  a.omega = st.omega;
  a.phase = st.phase;
  a.F = pl.F;
  a.F4 = pl.F4;
  a.N4 = pl.N4;
  a.Sp = pl.Sp;
  a.eta2 = tr.cp.eta2;
  a.chunk = tl.chunk;
  a.part = tl.nchunk > 1 ? (double*)st.part : (double*)st.out;  // one chunk: its partials ARE the results
  a.mpad = tl.mpad;
  const dim3 grid((unsigned)tl.pt, (unsigned)pl.ndb, (unsigned)tl.nchunk);
  ev_begin(e, e->stream, EV_PATHS, 2.0 * (double)tl.mc * (double)(a.N + pl.F) * pl.Sp, (int)tl.pt, (int)tl.nchunk, pl.S, train ? 1 : 0);
  const bool known = with_kind_nc(tr.cp.kind, e->nc_pad, [&](auto kind, auto nc) {
    hipLaunchKernelGGL((paths_eval_kernel<decltype(kind)::value, decltype(nc)::value>), grid, dim3(64), 0, e->stream, a);
  });
  if (known && tl.nchunk > 1)
    hipLaunchKernelGGL(paths_eval_finish_kernel, dim3((unsigned)(((int64_t)pl.S * tl.mpad + 255) / 256)), dim3(256), 0, e->stream,
                       (const double*)st.part, (int32_t)tl.nchunk, pl.Sp, pl.S, tl.mpad, (double*)st.out);
  ev_end(e);
  if (!known) return fail(e, GMB_EINVAL, "unknown kernel kind %d", tr.cp.kind);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

// what the two evaluation calls ask: a prepared state of the factor's current epoch
int paths_ready(gmb_engine* e, const char* what) {
  if (!e) return GMB_EINVAL;
  if (!e->paths.ready) return fail(e, GMB_EINVAL, "%s: no paths are prepared: call gmb_paths_prepare first", what);
  if (e->paths.epoch != e->fs.epoch() || !e->have_theta || e->terms.empty())
    return fail(e, GMB_EINVAL, "%s: the prepared paths are stale (the data, theta or the factor changed since gmb_paths_prepare): prepare them again", what);
  return GMB_OK;
}

// the plan's bytes against the device, then the allocation (`buffers`: the call's list over a visitor)
extern "C++" template <typename Buffers>
int paths_reserve(gmb_engine* e, const char* what, Buffers&& buffers) {
  int rc;
  Budget need;
  buffers(need);
  double free_b;
  if ((rc = device_free_bytes(e, &free_b))) return rc;
  if (need.fresh > free_b)
    return fail(e, GMB_ENOMEM, "%s needs %.0f bytes on the device, %.0f more than it holds for the engine now; %.0f bytes are free -- nothing was computed",
                what, need.total, need.fresh, free_b);
  Reserver take{e->pool};
  buffers(take);
  return take.rc;
}

}  // namespace

int gmb_paths_prepare(gmb_engine* e, int32_t S, int32_t F, const double* omega, const double* phase, const double* w, const double* eps) {
  const char* what = "gmb_paths_prepare";
  if (!e) return GMB_EINVAL;
  if (e->solve_hook || e->dist_mode != 0)  // (said before readiness: switching the mode has already dropped the factor)
    return fail(e, GMB_EINVAL, "%s is not available on distributed engines (gmb_dist_*, capacity mode): factorise with gmb_factorize on one device", what);
  int rc = joint_ready(e, what);
  if (rc) return rc;
  const gmb_kernel_spec& sp = e->spec;
  if (sp.additive || e->terms.size() != 1)
    return fail(e, GMB_EINVAL, "%s: additive models are not supported (one stationary term over the continuous dimensions only)", what);
  if (e->periodic) return fail(e, GMB_EINVAL, "%s: periodic models are not supported (their prior features are warped inputs)", what);
  if (sp.n_lin > 0) return fail(e, GMB_EINVAL, "%s: linear dimensions are not supported (their prior features are finite linear features)", what);
  if (spec_ntab(sp) > 0)
    return fail(e, GMB_EINVAL, "%s: coregion tables (categorical dimensions or an output column) are not supported", what);
  if (S < 1 || S > PATHS_MAX_S) return fail(e, GMB_EINVAL, "%s: S = %d draws (1 <= S <= %d is required)", what, (int)S, PATHS_MAX_S);
  if (F < 1 || F > PATHS_MAX_F) return fail(e, GMB_EINVAL, "%s: F = %d features (1 <= F <= %d is required)", what, (int)F, PATHS_MAX_F);
  if (!omega || !phase || !w || !eps) return fail(e, GMB_EINVAL, "%s: omega, phase, w and eps must not be NULL", what);
  HIP_TRY(e, hipSetDevice(e->device));
  PathState& st = e->paths;
  const gmb_engine::Term& tr = e->terms[0];
  PathsPlan pl;  // the features alone, at the training points
  if (pl.make(0, F, e->N, S)) return fail(e, GMB_EINVAL, "%s: S = %d, F = %d behind N = %lld is more than a call takes", what, (int)S, (int)F, (long long)e->N);
  const int64_t mrow = round_up(S, TILE);  // the draws as the test index of a prediction's V
  if ((rc = paths_reserve(e, what, [&](auto& v) { paths_prepare_buffers(*e, st, pl, (double)mrow, v); }))) return rc;
  st.clear();  // from here on the previous draws are gone
  // the host's part: frequencies by prepared column, phases, weights scaled by eta sqrt(2 / F) and laid draw-fastest
  const int nc = tr.pa.nc, ncp = e->nc_pad;
  std::vector<double> hom((size_t)ncp * pl.F4, 0.0), hph((size_t)pl.F4, 0.0), hwt((size_t)pl.F4 * pl.Sp, 0.0);
  const double scale = tr.eta * std::sqrt(2.0 / (double)F);
  for (int64_t f = 0; f < F; ++f) {
    for (int k = 0; k < nc; ++k) hom[(size_t)k * pl.F4 + f] = omega[f * nc + k];
    hph[f] = phase[f];
    for (int s = 0; s < S; ++s) hwt[(size_t)f * pl.Sp + s] = scale * w[(int64_t)s * F + f];
  }
  HIP_TRY(e, hipMemcpyAsync(st.omega, hom.data(), hom.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemcpyAsync(st.phase, hph.data(), hph.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemcpyAsync(st.wt, hwt.data(), hwt.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemcpyAsync(st.eps, eps, (size_t)S * e->N * sizeof(double), hipMemcpyHostToDevice, e->stream));
  reset_predict_timings(e);
  e->tm.predict_gemm_form = 0;  // the right-hand sides are solved for, as in gmb_predict_with_grad: neither dW nor U is touched
  const double d = std::sqrt(tr.cp.sigma2 + tr.cp.jitter);  // exactly the diagonal the covariance build adds to K
  PhaseTimer tp(e);
  auto work = [&]() -> int {
    for (int64_t t = 0; t < pl.ntile; ++t) {  // R = y - Phi(X) w~ - d eps, draw index fastest, into the prediction's V
      const PathsTile tl = pl.tile(t);
      if ((rc = paths_eval_tile(e, pl, tl, e->pts.xs + tl.first, e->Nr, false))) return rc;
      hipLaunchKernelGGL(paths_resid_kernel, dim3((unsigned)((mrow * tl.mc + 255) / 256)), dim3(256), 0, e->stream, (const double*)st.out, tl.mpad,
                         (const double*)e->dy, (const double*)st.eps, e->N, S, d, tl.first, tl.mc, (double*)e->pw.dV, mrow);
    }
    if (e->Np > e->N) HIP_TRY(e, hipMemsetAsync(e->pw.dV + e->N * mrow, 0, (size_t)((e->Np - e->N) * mrow) * sizeof(double), e->stream));
    HIP_TRY(e, hipGetLastError());
    if ((rc = predict_solve_v(e, mrow, false))) return rc;  // R L^-T ...
    if ((rc = predict_solve_w(e, mrow))) return rc;         // ... L^-1 = (Sigma^-1 R)^T
    hipLaunchKernelGGL(paths_store_a_kernel, dim3((unsigned)((e->Np * pl.Sp + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->pw.dV, mrow,
                       e->N, e->Np, S, pl.Sp, (double*)st.A);
    HIP_TRY(e, hipGetLastError());
    return GMB_OK;
  };
  rc = predict_end(e, &tp, work());  // (drains the stream: the host vectors above and the caller's eps have been read)
  if (rc) return rc;
  st.ready = true;
  st.epoch = e->fs.epoch();
  st.S = S, st.Sp = pl.Sp, st.F = F, st.F4 = pl.F4;
  return GMB_OK;
}

int gmb_paths_eval(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, double* Y, int64_t ldy, int32_t memspace) {
  const char* what = "gmb_paths_eval";
  int rc = paths_ready(e, what);
  if (rc) return rc;
  if (M < 0 || (M > 0 && (!Xs || !Y)) || ldxs < e->D || ldy < M)
    return fail(e, GMB_EINVAL, "%s: bad M/Xs/ldxs/Y/ldy (M >= 0, ldxs >= D, ldy >= M, no NULL array)", what);
  if (M == 0) return GMB_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  PathState& st = e->paths;
  PathsPlan pl;
  if (pl.make(e->N, st.F, M, st.S)) return fail(e, GMB_EINVAL, "%s: M = %lld points are more than a call takes (M <= 2^40)", what, (long long)M);
  if ((rc = paths_reserve(e, what, [&](auto& v) { paths_eval_buffers(*e, st, pl, v); }))) return rc;
  reset_predict_timings(e);
  const CopyKinds ck = copy_kinds(memspace);
  const size_t row = e->D * sizeof(double);
  PhaseTimer tp(e);
  auto tiles = [&]() -> int {
    for (int64_t t = 0; t < pl.ntile; ++t) {
      const PathsTile tl = pl.tile(t);
      HIP_TRY(e, hipMemcpy2DAsync(e->pg.Xs, row, Xs + tl.first * ldxs, ldxs * sizeof(double), row, tl.mc, ck.in, e->stream));
      if ((rc = prep_points(e, e->pg.Xs, tl.mc, e->D, tl.mpad, e->pg.xs, e->pg.xl, e->pg.cat, &e->terms[0].pa))) return rc;
      if ((rc = paths_eval_tile(e, pl, tl, e->pg.xs, tl.mpad, true))) return rc;
      if (hipMemcpy2DAsync(Y + tl.first, ldy * sizeof(double), st.out, tl.mpad * sizeof(double), tl.mc * sizeof(double), st.S, ck.out, e->stream) != hipSuccess)
        return fail(e, GMB_EHIP, "%s: copying the draws out failed", what);
    }
    return GMB_OK;
  };
  return predict_end(e, &tp, tiles());
}

int gmb_paths_eval_own(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, const int32_t* draw, double* val, double* grad, int64_t ldg,
                       int32_t memspace) {
  const char* what = "gmb_paths_eval_own";
  int rc = paths_ready(e, what);
  if (rc) return rc;
  if (M < 0 || (M > 0 && (!Xs || !draw || !val)) || ldxs < e->D || (grad && ldg < e->D))
    return fail(e, GMB_EINVAL, "%s: bad M/Xs/ldxs/draw/val/ldg (M >= 0, ldxs >= D, ldg >= D, no NULL array but grad)", what);
  if (M == 0) return GMB_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  PathState& st = e->paths;
  {  // every point's draw exists: looked at on the host before anything is launched
    std::vector<int32_t> staged;
    const int32_t* hd = draw;
    if (memspace == GMB_DEVICE) {
      staged.resize((size_t)M);
      HIP_TRY(e, hipMemcpy(staged.data(), draw, (size_t)M * sizeof(int32_t), hipMemcpyDeviceToHost));
      hd = staged.data();
    }
    for (int64_t m = 0; m < M; ++m)
      if (hd[m] < 0 || hd[m] >= st.S)
        return fail(e, GMB_EINVAL, "%s: draw[%lld] = %d is outside [0, %d)", what, (long long)m, (int)hd[m], (int)st.S);
  }
  PathsPlan pl;
  if (pl.make(e->N, st.F, M, st.S)) return fail(e, GMB_EINVAL, "%s: M = %lld points are more than a call takes (M <= 2^40)", what, (long long)M);
  if ((rc = paths_reserve(e, what, [&](auto& v) { paths_own_buffers(*e, st, pl, v); }))) return rc;
  reset_predict_timings(e);
  const CopyKinds ck = copy_kinds(memspace);
  const size_t row = e->D * sizeof(double);
  const gmb_engine::Term& tr = e->terms[0];
  PhaseTimer tp(e);
  auto tiles = [&]() -> int {
    for (int64_t t = 0; t < pl.ntile; ++t) {
      const PathsTile tl = pl.tile(t);
      HIP_TRY(e, hipMemcpy2DAsync(e->pg.Xs, row, Xs + tl.first * ldxs, ldxs * sizeof(double), row, tl.mc, ck.in, e->stream));
      HIP_TRY(e, hipMemcpyAsync(st.draw, draw + tl.first, (size_t)tl.mc * sizeof(int32_t), ck.in, e->stream));
      if ((rc = prep_points(e, e->pg.Xs, tl.mc, e->D, tl.mpad, e->pg.xs, e->pg.xl, e->pg.cat, &tr.pa))) return rc;
      if (grad) HIP_TRY(e, hipMemsetAsync(e->pg.grad, 0, (size_t)(tl.mc * e->D) * sizeof(double), e->stream));
      PathsOwnArgs a{};
      a.txs = e->pg.xs;
      a.mpad = tl.mpad;
      a.mc = tl.mc;
      a.draw = st.draw;
      a.xs = e->pts.xs;
      a.npad = e->Nr;
      a.N = e->N;
      a.A = st.A;
      a.wt = st.wt;
      a.omega = st.omega;
      a.phase = st.phase;
      a.F = pl.F;
      a.F4 = pl.F4;
      a.N4 = pl.N4;
      a.Sp = pl.Sp;
      a.eta2 = tr.cp.eta2;
      a.chunk = tl.own_chunk;
      a.part = st.part;
      const dim3 grid((unsigned)(tl.mpad / PATHS_OWN_PTS), (unsigned)tl.own_nchunk);
      ev_begin(e, e->stream, EV_PATHS, 0.0, (int)(tl.mpad / PATHS_OWN_PTS), (int)tl.own_nchunk, st.S, 2);
      const bool known = with_kind_nc(tr.cp.kind, e->nc_pad, [&](auto kind, auto nc) {
        hipLaunchKernelGGL((paths_own_kernel<decltype(kind)::value, decltype(nc)::value>), grid, dim3(256), 0, e->stream, a);
      });
      if (!known) {
        ev_end(e);
        return fail(e, GMB_EINVAL, "unknown kernel kind %d", tr.cp.kind);
      }
      PathsOwnFinishArgs f{};
      f.part = st.part;
      f.nchunk = (int32_t)tl.own_nchunk;
      f.nc = tr.pa.nc;
      f.nc_pad = e->nc_pad;
      f.D = e->D;
      f.mpad = tl.mpad;
      f.mc = tl.mc;
      for (int k = 0; k < tr.pa.nc; ++k) f.idx_cont[k] = tr.pa.idx_cont[k], f.scale[k] = 2.0 * tr.pa.inv_ls[k];
      f.val = st.val;
      f.grad = grad ? (double*)e->pg.grad : nullptr;
      hipLaunchKernelGGL(paths_own_finish_kernel, dim3((unsigned)((tl.mc + 255) / 256)), dim3(256), 0, e->stream, f);
      ev_end(e);
      HIP_TRY(e, hipGetLastError());
      if (hipMemcpyAsync(val + tl.first, st.val, (size_t)tl.mc * sizeof(double), ck.out, e->stream) != hipSuccess ||
          (grad && hipMemcpy2DAsync(grad + tl.first * ldg, ldg * sizeof(double), e->pg.grad, row, row, tl.mc, ck.out, e->stream) != hipSuccess))
        return fail(e, GMB_EHIP, "%s: copying the results out failed", what);
    }
    return GMB_OK;
  };
  return predict_end(e, &tp, tiles());
}

int gmb_paths_clear(gmb_engine* e) {
  if (!e) return GMB_EINVAL;
  PathState& st = e->paths;
  st.clear();
  st.A.drop(e->pool), st.wt.drop(e->pool), st.omega.drop(e->pool), st.phase.drop(e->pool);
  st.out.drop(e->pool), st.part.drop(e->pool), st.val.drop(e->pool), st.eps.drop(e->pool), st.draw.drop(e->pool);
  return GMB_OK;
}

int32_t gmb_paths_count(gmb_engine* e) { return e && e->paths.ready ? e->paths.S : 0; }

int64_t gmb_debug_paths_plan(int64_t N, int64_t F, int64_t M, int64_t S, int32_t nacc, int64_t* out, int64_t cap) {
  return paths_plan_dump(N, F, M, S, nacc, out, cap);
}

int gmb_predict_joint(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise, double jitter,
                      double* mean, double* cov, int64_t ldc, int32_t memspace) {
  return predict_joint_sel(e, nullptr, "gmb_predict_joint", Xs, M, ldxs, with_noise, jitter, mean, cov, ldc, memspace);
}

int gmb_predict_joint_terms(gmb_engine* e, uint32_t terms, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise, double jitter,
                            double* mean, double* cov, int64_t ldc, int32_t memspace) {
  return predict_joint_sel(e, &terms, "gmb_predict_joint_terms", Xs, M, ldxs, with_noise, jitter, mean, cov, ldc, memspace);
}

int gmb_draw_joint(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise, double jitter,
                   const double* Z, int64_t S, int64_t ldz, double* Y, int64_t ldy, double* mean, int32_t memspace) {
  return draw_joint_sel(e, nullptr, "gmb_draw_joint", Xs, M, ldxs, with_noise, jitter, Z, S, ldz, Y, ldy, mean, memspace);
}

int gmb_draw_joint_terms(gmb_engine* e, uint32_t terms, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise, double jitter,
                         const double* Z, int64_t S, int64_t ldz, double* Y, int64_t ldy, double* mean, int32_t memspace) {
  return draw_joint_sel(e, &terms, "gmb_draw_joint_terms", Xs, M, ldxs, with_noise, jitter, Z, S, ldz, Y, ldy, mean, memspace);
}

int gmb_num_terms(const gmb_engine* e) {
  if (!e || !e->have_theta || e->terms.empty()) return GMB_EINVAL;
  return (int)e->terms.size();
}

int gmb_predict_decompose(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, double* means, int64_t ldm, double* cov,
                          int64_t ldcv, double* noise, int32_t memspace) {
  int rc = joint_ready(e, "gmb_predict_decompose");
  if (rc) return rc;
  if (M < 0 || (M > 0 && (!Xs || !means || !cov)) || ldxs < e->D || ldm < M || ldcv < M)
    return fail(e, GMB_EINVAL, "bad Xs/M/ldxs/means/ldm/cov/ldcv");
  if (M == 0) return GMB_OK;
  const int T = (int)e->terms.size();
  if (T > TG_MAX_TERMS) return fail(e, GMB_EINVAL, "gmb_predict_decompose: %d terms (at most %d)", T, TG_MAX_TERMS);
  HIP_TRY(e, hipSetDevice(e->device));
  reset_predict_timings(e);
  e->tm.predict_gemm_form = 0;  // the stacked V is always solved for, as in gmb_predict_with_grad: neither dW nor U is touched
  const int64_t Mt = decompose_tile_rows(e, M);
  const int nchunk = red_chunks(e->N);
  // every allocation before the first launch: T stacked blocks in the prediction's workspace, the partials, the results
  if ((rc = predict_workspace(e, (int64_t)T * Mt))) return rc;
  if ((rc = e->tg.reserve(e->pool, Mt, (int64_t)nchunk * tg_entries(T)))) return rc;
  const CopyKinds ck = copy_kinds(memspace);
  const int np = T * (T + 1) / 2;
  PhaseTimer tp(e);
  auto tiles = [&]() -> int {
    for (int64_t m0 = 0; m0 < M; m0 += Mt) {
      const int64_t mc = std::min<int64_t>(Mt, M - m0);
      const int64_t mpad = round_up(mc, TILE);
      if ((rc = decompose_tile(e, Xs + m0 * ldxs, mc, mpad, ldxs, ck.in))) return rc;
      const double* dmeans = e->tg.out;
      const double* dcov = dmeans + (int64_t)T * mpad;
      const double* dnoise = dcov + (int64_t)np * mpad;
      if (hipMemcpy2DAsync(means + m0, ldm * sizeof(double), dmeans, mpad * sizeof(double), mc * sizeof(double), T, ck.out, e->stream) != hipSuccess ||
          hipMemcpy2DAsync(cov + m0, ldcv * sizeof(double), dcov, mpad * sizeof(double), mc * sizeof(double), np, ck.out, e->stream) != hipSuccess ||
          (noise && hipMemcpyAsync(noise + m0, dnoise, mc * sizeof(double), ck.out, e->stream) != hipSuccess))
        return fail(e, GMB_EHIP, "gmb_predict_decompose: copying the results out failed");
    }
    return GMB_OK;
  };
  return predict_end(e, &tp, tiles());
}

int gmb_loo(gmb_engine* e, int64_t i0, int64_t n, int32_t with_noise, double* mean, double* var, int32_t memspace) {
  return loo_impl(e, i0, n, with_noise, mean, var, memspace);
}

int gmb_leave_out(gmb_engine* e, const int64_t* idx, int64_t m, int32_t with_noise, double* mean, double* var, double* cov, int64_t ldc,
                  int32_t memspace) {
  return leave_out_impl(e, idx, m, with_noise, mean, var, cov, ldc, memspace);
}

int gmb_predict_groups(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, const int64_t* offsets, int64_t G, const double* weights,
                       double* mean, double* var, double* cov, int64_t ldc, int32_t memspace) {
  return predict_groups_sel(e, nullptr, "gmb_predict_groups", Xs, M, ldxs, offsets, G, weights, mean, var, cov, ldc, memspace);
}

int gmb_predict_groups_terms(gmb_engine* e, uint32_t terms, const double* Xs, int64_t M, int64_t ldxs, const int64_t* offsets, int64_t G,
                             const double* weights, double* mean, double* var, double* cov, int64_t ldc, int32_t memspace) {
  return predict_groups_sel(e, &terms, "gmb_predict_groups_terms", Xs, M, ldxs, offsets, G, weights, mean, var, cov, ldc, memspace);
}

int gmb_predict_slope(gmb_engine* e, const double* Xs, int64_t M, int64_t ldxs, double* dmean, double* dvar, int64_t ldg, double* dcov,
                      int64_t ldc, int32_t memspace) {
  return predict_slope_sel(e, nullptr, "gmb_predict_slope", Xs, M, ldxs, dmean, dvar, ldg, dcov, ldc, memspace);
}

int gmb_predict_slope_terms(gmb_engine* e, uint32_t terms, const double* Xs, int64_t M, int64_t ldxs, double* dmean, double* dvar,
                            int64_t ldg, double* dcov, int64_t ldc, int32_t memspace) {
  return predict_slope_sel(e, &terms, "gmb_predict_slope_terms", Xs, M, ldxs, dmean, dvar, ldg, dcov, ldc, memspace);
}

int64_t gmb_debug_slope_tile_rows(int64_t Np, int32_t Dc) {
  if (Np < 1 || Dc < 1 || Dc > SLOPE_MAX_COLS) return GMB_EINVAL;
  return slope_tile_rows(slope_predict_rows_max(Np), Dc);
}

int gmb_design_batch(gmb_engine* e, const double* Xc, int64_t M, int64_t ldc, const double* Xr, int64_t R, int64_t ldr, const double* w,
                     int32_t q, int32_t with_noise, int32_t allow_repeats, int64_t* picks, double* gains, double* score0, double* ivar0,
                     int32_t memspace) {
  return design_batch_impl(e, Xc, M, ldc, Xr, R, ldr, w, q, with_noise, allow_repeats, picks, gains, score0, ivar0, memspace);
}

int64_t gmb_debug_design_plan(int64_t Np, int64_t M, int64_t R, int64_t* out, int64_t cap) { return design_plan_dump(Np, M, R, out, cap); }

int64_t gmb_debug_group_tasks(const int64_t* offsets, int64_t G, int64_t chunk, int64_t* out, int64_t cap) {
  if (!offsets || G < 1) return (int64_t)GMB_EINVAL;
  if (group_check_offsets(offsets, G, offsets[G], nullptr)) return (int64_t)GMB_EINVAL;
  std::vector<int64_t> tasks;
  const int64_t n = group_build_tasks(offsets, G, chunk > 0 ? chunk : GROUP_CHUNK, &tasks);
  for (int64_t i = 0; i < n && i < cap && out; ++i)
    for (int k = 0; k < 3; ++k) out[3 * i + k] = tasks[(size_t)(3 * i + k)];
  return n;
}

int gmb_copy_factor(const gmb_engine* ce, int64_t r0, int64_t nr, int64_t c0, int64_t nc, double* out) {
  gmb_engine* e = const_cast<gmb_engine*>(ce);
  if (!e || !out) return GMB_EINVAL;
  if (e->fs.valid() && require_full_factor(e, "gmb_copy_factor")) return GMB_EINVAL;
  if (!e->dA || e->dA.cap <= 0 || r0 < 0 || c0 < 0 || nr < 0 || nc < 0 || r0 + nr > e->Nr || c0 + nc > e->Np)
    return fail(e, GMB_EINVAL, "factor window out of range");
  if (nr == 0 || nc == 0) return GMB_OK;
  std::vector<double> tmp((size_t)nr * nc);  // column-major window
  HIP_TRY(e, hipMemcpy2D(tmp.data(), nr * sizeof(double), e->dA + r0 + c0 * e->ld, e->ld * sizeof(double),
                         nr * sizeof(double), nc, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < nr; ++i)
    for (int64_t j = 0; j < nc; ++j) out[i * nc + j] = tmp[(size_t)j * nr + i];
  return GMB_OK;
}

int gmb_copy_v(const gmb_engine* ce, double* out) {
  gmb_engine* e = const_cast<gmb_engine*>(ce);
  int rc = require_ready(e, true);
  if (rc) return rc;
  HIP_TRY(e, hipMemcpy(out, e->dv, e->N * sizeof(double), hipMemcpyDeviceToHost));
  return GMB_OK;
}

int gmb_copy_alpha(const gmb_engine* ce, double* out) {
  gmb_engine* e = const_cast<gmb_engine*>(ce);
  int rc = require_ready(e, false);
  if (rc) return rc;
  if (!out) return fail(e, GMB_EINVAL, "null output");
  if (!e->fs.gradient_alpha() || !e->dalpha)  // (the mark alone: an invalidating call leaves the previous alpha readable)
    return fail(e, GMB_EINVAL, "alpha exists only after a gradient evaluation (gmb_nlml with grad)");
  HIP_TRY(e, hipMemcpy(out, e->dalpha, e->N * sizeof(double), hipMemcpyDeviceToHost));
  return GMB_OK;
}

int gmb_ls_limits(int32_t device, const double* X, int64_t N, int32_t n_cols, int64_t ldx, int32_t ard,
                  double* lower, double* upper) {
  if (!X || !lower || !upper || N < 1 || n_cols < 1 || n_cols > GMB_MAX_DIMS || ldx < n_cols)
    return GMB_EINVAL;
  int nd = gmb_device_count();
  if (nd < 0) return GMB_ENODEVICE;
  if (device < 0 || device >= nd) return GMB_EINVAL;
  if (hipSetDevice(device) != hipSuccess) return GMB_EHIP;
  const int64_t npad = round_up(N, TILE);
  const int ngroups = ard ? n_cols : 1, gw = ard ? 1 : n_cols;
  std::vector<double> soa((size_t)n_cols * npad, 0.0);
  for (int64_t i = 0; i < N; ++i)
    for (int k = 0; k < n_cols; ++k) soa[(size_t)k * npad + i] = X[i * ldx + k];
  double* dpts = nullptr;
  unsigned long long *dmn = nullptr, *dmx = nullptr;
  int rc = GMB_OK;
  std::vector<unsigned long long> hmn(ngroups, ~0ull), hmx(ngroups, 0ull);
  if (hipMalloc((void**)&dpts, soa.size() * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&dmn, ngroups * sizeof(unsigned long long)) != hipSuccess ||
      hipMalloc((void**)&dmx, ngroups * sizeof(unsigned long long)) != hipSuccess) {
    rc = GMB_ENOMEM;
  } else if (hipMemcpy(dpts, soa.data(), soa.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
             hipMemcpy(dmn, hmn.data(), ngroups * sizeof(unsigned long long), hipMemcpyHostToDevice) != hipSuccess ||
             hipMemcpy(dmx, hmx.data(), ngroups * sizeof(unsigned long long), hipMemcpyHostToDevice) != hipSuccess) {
    rc = GMB_EHIP;
  } else {
    const int tiles = (int)(npad / TILE);
    const int64_t npairs = (int64_t)tiles * (tiles + 1) / 2;
    hipLaunchKernelGGL(ls_limits_kernel, dim3((unsigned)npairs, ngroups), dim3(256), 0, 0, dpts, N, npad, gw,
                       dmn, dmx, tiles);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(hmn.data(), dmn, ngroups * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(hmx.data(), dmx, ngroups * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
      rc = GMB_EHIP;
  }
  if (dpts) (void)hipFree(dpts);
  if (dmn) (void)hipFree(dmn);
  if (dmx) (void)hipFree(dmx);
  if (rc) return rc;
  for (int g = 0; g < ngroups; ++g) {
    if (hmn[g] == ~0ull) {
      lower[g] = -1.0;
      upper[g] = -1.0;
    } else {
      double lo, hi;
      memcpy(&lo, &hmn[g], 8);
      memcpy(&hi, &hmx[g], 8);
      lower[g] = std::sqrt(lo);
      upper[g] = std::sqrt(hi);
    }
  }
  return GMB_OK;
}

// Register-only MFMA loop, launched back to back until `seconds` have passed (at least once): per-launch HIP
// events give the rate, block 0's s_memtime span over its own loop gives the shader clock.
static int mfma_f64_run(int32_t device, double seconds, int iters, double* mean_tf, double* min_tf, double* mhz,
                        double* cyc_per_mfma, int64_t* launches) {
  int nd = gmb_device_count();
  if (nd < 0) return GMB_ENODEVICE;
  if (device < 0 || device >= nd) return GMB_EINVAL;
  if (hipSetDevice(device) != hipSuccess) return GMB_EHIP;
  double* sink = nullptr;
  if (hipMalloc((void**)&sink, 16) != hipSuccess) return GMB_ENOMEM;
  hipEvent_t a, b;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  const int blocks = 256 * 2;  // two workgroups per compute unit, as the GEMM runs
  hipLaunchKernelGGL(mfma_f64_peak_kernel, dim3(blocks), dim3(256), 0, 0, sink, 100, 1.0);  // warm-up
  const double flops = (double)blocks * 4.0 * (double)iters * 16.0 * 2.0 * 16 * 16 * 4;
  double sum_ms = 0.0, worst_ms = 0.0, sum_mhz = 0.0, sum_cyc = 0.0;
  int64_t n = 0;
  int rc = GMB_OK;
  do {
    (void)hipEventRecord(a, 0);
    hipLaunchKernelGGL(mfma_f64_peak_kernel, dim3(blocks), dim3(256), 0, 0, sink, iters, 1.0);
    (void)hipEventRecord(b, 0);
    if (hipEventSynchronize(b) != hipSuccess || hipGetLastError() != hipSuccess) {
      rc = GMB_EHIP;
      break;
    }
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, a, b);
    double hsink[2] = {0.0, 0.0};
    if (hipMemcpy(hsink, sink, 16, hipMemcpyDeviceToHost) != hipSuccess) {
      rc = GMB_EHIP;
      break;
    }
    sum_ms += ms;
    worst_ms = std::max(worst_ms, (double)ms);
    // block 0's loop spans (almost) the whole launch.  s_memtime ticks once per TWO shader cycles on gfx950
    // (measured: 1187 MHz of counter beside 77.8 TFLOP/s, i.e. 2375 MHz of matrix-pipe issue at 64 cycles per MFMA)
    sum_mhz += 2.0 * hsink[1] / ((double)ms * 1e3);
    sum_cyc += hsink[1] / ((double)iters * 16.0);
    ++n;
  } while (sum_ms < seconds * 1e3);
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  (void)hipFree(sink);
  if (rc) return rc;
  if (mean_tf) *mean_tf = flops * (double)n / (sum_ms * 1e-3) / 1e12;
  if (min_tf) *min_tf = flops / (worst_ms * 1e-3) / 1e12;
  if (mhz) *mhz = sum_mhz / (double)n;
  if (cyc_per_mfma) *cyc_per_mfma = sum_cyc / (double)n;
  if (launches) *launches = n;
  return GMB_OK;
}

int gmb_mfma_f64_peak(int32_t device, double* tflops, double* cycles_per_mfma) {
  if (!tflops) return GMB_EINVAL;
  return mfma_f64_run(device, 0.0, 2000, tflops, nullptr, nullptr, cycles_per_mfma, nullptr);
}

int gmb_mfma_f64_sustained(int32_t device, double seconds, double* mean_tflops, double* min_tflops, double* shader_mhz,
                           int64_t* launches) {
  if (!mean_tflops || !(seconds >= 0.0) || seconds > 60.0) return GMB_EINVAL;
  return mfma_f64_run(device, seconds, 40000, mean_tflops, min_tflops, shader_mhz, nullptr, launches);  // ~37 ms per launch
}

// ---- block-level operations (multi-GPU driver) ---------------------------------------------
// Host-only (no device): the tile list of one GEMM launch as the kernels enumerate it -- gemm_schedule's
// grid, then gemm_decode_tile for every block.  out receives (block, tm, tn) triples of the blocks that
// compute a tile; returns their number (or the negative status).  Tests check that every computed tile of
// the (triangular, strided, strip-ordered ...) launch appears exactly once.
int64_t gmb_debug_tile_list(int32_t mt, int32_t nt, int32_t bm, int32_t bn, int32_t k, int32_t tri, int32_t tri_off,
                            int32_t nblk_stride, int32_t klo_n, int32_t khi_n, int32_t order, int32_t strip,
                            int32_t* out, int64_t cap, int32_t* grid) {
  if (mt < 1 || nt < 1 || k < KT || nblk_stride < 1 || (bm != 128 && bm != 64) || (bn != 128 && bn != 64 && bn != 32))
    return GMB_EINVAL;
  GemmArgs g{};
  g.mt = mt;
  g.nt = nt;
  g.k = k;
  g.tri = tri;
  g.tri_off = tri_off;
  g.nblk_stride = nblk_stride;
  g.klo_n = klo_n;
  g.khi_n = khi_n;
  g.order = order;
  g.strip = order == 0 ? strip : 0;
  double flops = 0.0;
  const int nblocks = gemm_schedule(g, bm, bn, &flops);
  if (grid) *grid = nblocks;
  int64_t n = 0;
  for (int b = 0; b < nblocks; ++b) {
    int tm = -1, tn = -1;
    if (!gemm_decode_tile(g, bm, bn, b, tm, tn)) continue;
    if (out && n < cap) {
      out[3 * n] = b;
      out[3 * n + 1] = tm;
      out[3 * n + 2] = tn;
    }
    ++n;
  }
  return n;
}

int64_t gmb_debug_cov_grid(int32_t ti, int32_t tj, int32_t strip, int32_t tri_grid, int32_t row_first, int32_t row_stride,
                           int32_t keep_order, int32_t* out, int64_t cap, int64_t* grid) {
  if (ti < 1 || tj < 1 || strip < 1 || row_first < 0 || row_stride < 0) return GMB_EINVAL;
  const long long nb = cov_grid_blocks(ti, tj, strip, tri_grid, row_first, row_stride);
  if (grid) *grid = nb;
  int64_t n = 0;
  for (long long b = 0; b < nb; ++b) {
    int tix, lo, hi;
    if (!cov_decode_block(ti, tj, strip, tri_grid, row_first, row_stride, keep_order != 0, b, &tix, &lo, &hi)) continue;
    for (int t = lo; t < hi; ++t) {
      if (out && n < cap) {
        out[3 * n] = (int32_t)b;
        out[3 * n + 1] = tix;
        out[3 * n + 2] = t;
      }
      ++n;
    }
  }
  return n;
}

int64_t gmb_debug_chol_task(int32_t t, int32_t nct, int32_t nrt, int32_t* I, int32_t* J) {
  if (nct < 1 || nrt < nct) return GMB_EINVAL;
  const int n = ct_task_count(nct, nrt);
  int i = -1, j = -1;
  if (t >= 0 && t < n) ct_decode(t, nct, nrt, i, j);
  if (I) *I = i;
  if (J) *J = j;
  return n;
}

int64_t gmb_chol_task_trace(gmb_engine* e, int32_t enable, uint64_t* out, int64_t cap_tasks) {
  if (!e) return GMB_EINVAL;
  if (enable >= 0) e->ct_trace = enable != 0;
  // only the stamps of the LAST factorisation count: 0 when it did not run on the tile kernel or ran untraced
  const int64_t n = (e->chol.tiles && e->chol.traced && e->dct_trace && e->dct_trace.cap >= 4 * (int64_t)e->chol.ntasks) ? e->chol.ntasks : 0;
  if (out && n > 0) {
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(out, e->dct_trace, (size_t)std::min<int64_t>(n, cap_tasks) * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  return n;
}

int gmb_debug_chol_lose_tickets(gmb_engine* e, int32_t n) {
  if (!e || n < 0) return GMB_EINVAL;
  e->ct_lose = n;
  return GMB_OK;
}

int gmb_debug_assume_factored(gmb_engine* e) {
  if (!e) return GMB_EINVAL;
  // a door for the timing tools (tools/gpu_dist_emulate.py), never for a caller of the product: it takes an explicit opt-in
  // in the environment
  const char* door = getenv("GUMBI_HIP_DEBUG_DOORS");
  if (!door || door[0] != '1') return fail(e, GMB_EINVAL, "gmb_debug_assume_factored needs GUMBI_HIP_DEBUG_DOORS=1 in the environment");
  if (e->fs.none() || !e->have_theta) return fail(e, GMB_EINVAL, "no factorisation has been attempted at this theta");
  e->fs.assume_factored();
  e->notpd = -1;
  if (!std::isfinite(e->logdet)) e->logdet = 0.0;
  if (!std::isfinite(e->vnorm2)) e->vnorm2 = 0.0;
  return GMB_OK;
}

int gmb_set_chol_scheme(gmb_engine* e, int32_t scheme) {
  if (!e) return GMB_EINVAL;
  if (!chol_scheme_valid(scheme)) return fail(e, GMB_EINVAL, "Cholesky scheme %d: valid are -1 (by size), 0, 2, 3, 4", scheme);
  const int old = e->chol_scheme;
  e->chol_scheme = scheme;
  return old + 1;  // previous scheme + 1: "by size" (-1) comes back as 0, so no valid answer collides with a (negative) status
}

int gmb_set_grad_scheme(gmb_engine* e, int32_t scheme, int32_t lag) {
  if (!e || scheme < -1 || scheme > 2) return GMB_EINVAL;
  const int old = e->grad_scheme;
  e->grad_scheme = scheme;
  if (lag >= 0) e->et_lag = lag;
  return old + 1;
}

int gmb_reserve(gmb_engine* e, int32_t gradient, int64_t M) {
  int rc = require_ready(e, false);
  if (rc) return rc;
  if (M < 0) return fail(e, GMB_EINVAL, "M must be >= 0");
  HIP_TRY(e, hipSetDevice(e->device));
  if ((rc = ensure_factor_buffer(e))) return rc;
  if (gradient) {
    if ((rc = e->dW.reserve(e->pool, e->Np * e->Np))) return rc;
    if ((rc = grad_workspace(e))) return rc;
  }
  if (M > 0 && (rc = predict_workspace(e, predict_tile_rows(e, M)))) return rc;
  HIP_TRY(e, hipDeviceSynchronize());
  return GMB_OK;
}

int gmb_set_predict_form(gmb_engine* e, int32_t form) {
  if (!e || form < -1 || form > 1) return GMB_EINVAL;
  const int old = e->predict_form;
  e->predict_form = form;
  return old + 1;
}

int gmb_set_eval_pairs(gmb_engine* e, int32_t mode) {
  if (!e || mode < -1 || mode > 1) return GMB_EINVAL;
  const int old = e->et_pairs;
  e->et_pairs = mode;
  return old + 1;
}

int64_t gmb_debug_eval_tasks(int32_t nct, int32_t nrt, int32_t with_chol, int32_t lag, uint32_t* out, int64_t cap) {
  if (nct < 1 || nrt < nct || nrt > 0x3fff || lag < 0 || with_chol < 0 || with_chol > 3) return GMB_EINVAL;
  std::vector<uint32_t> list;
  et_build_tasks(nct, nrt, (with_chol & 1) != 0, lag, list, (with_chol & 2) != 0);
  if (out)
    for (int64_t i = 0; i < (int64_t)list.size() && i < cap; ++i) out[i] = list[(size_t)i];
  return (int64_t)list.size();
}

int gmb_blk_covariance(gmb_engine* e, double* out, int64_t ldo) {
  int rc = require_ready(e, false);
  if (rc) return rc;
  if (!out || ldo < e->Nr) return fail(e, GMB_EINVAL, "gmb_blk_covariance: out is null or ldo < %lld", (long long)e->Nr);
  // the interior tiles go out as 16-byte stores (covariance.hpp: cov_interior_tile): two rows per lane
  if ((((uintptr_t)out) | (uintptr_t)(ldo * (int64_t)sizeof(double))) & 15u)
    return fail(e, GMB_EINVAL, "gmb_blk_covariance: out must be 16-byte aligned and ldo even (16-byte stores)");
  HIP_TRY(e, hipSetDevice(e->device));
  if ((rc = build_sigma(e, out, ldo))) return rc;
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return GMB_OK;
}

int gmb_blk_potrf(gmb_engine* e, double* Akk, int64_t lda, int32_t nvalid, double* dinv16,
                  double* logdet_accum, int32_t* info) {
  if (!e || !Akk || nvalid < 1 || nvalid > TILE || lda < TILE) return fail(e, GMB_EINVAL, "bad potrf block");
  HIP_TRY(e, hipSetDevice(e->device));
  LeafArgs a{};
  a.A = Akk;
  a.lda = lda;
  a.nvalid = nvalid;
  a.dinv16 = dinv16;
  a.logdet = logdet_accum;
  a.info = info ? info : e->dinfo;
  a.row0 = 0;
#ifdef GMB_TUNING
  a.dbg = getenv("GMB_LEAF_DBG") ? logdet_accum + 1 : nullptr;  // stamps after the log-det slot (tools/gpu_leaf_timing.py)
#else
  a.dbg = nullptr;
#endif
  return launch_leaf(e, e->stream, a);
}

int gmb_blk_invert(gmb_engine* e, const double* Lkk, int64_t lda, int32_t nvalid, const double* dinv16,
                   double* invLkk) {
  if (!e || !Lkk || !dinv16 || !invLkk || nvalid < 1 || nvalid > TILE || lda < TILE)
    return fail(e, GMB_EINVAL, "bad invert block");
  HIP_TRY(e, hipSetDevice(e->device));
  InvArgs ia{};
  ia.L = Lkk;
  ia.lda = lda;
  ia.blk_stride = 0;
  ia.dinv16 = dinv16;
  ia.invL = invLkk;
  ia.n = nvalid;
  hipLaunchKernelGGL(leaf_invert_kernel, dim3(1), dim3(256), 0, e->stream, ia);
  HIP_TRY(e, hipGetLastError());
  return GMB_OK;
}

int gmb_blk_trsm(gmb_engine* e, double* B, int64_t ldb, int64_t nrows, const double* Lkk, int64_t ldl,
                 const double* dinv16, int32_t nvalid) {
  if (!e || !B || !Lkk || !dinv16 || nrows < 0 || nrows % 16 || ldb < nrows || ldl < TILE || nvalid < 1 ||
      nvalid > TILE)
    return fail(e, GMB_EINVAL, "bad trsm arguments (rows must be a multiple of 16)");
  HIP_TRY(e, hipSetDevice(e->device));
  return launch_trsm_strip(e, e->stream, B, ldb, nrows, Lkk, ldl, dinv16, nvalid, EV_CHOL_STRIP);
}

int gmb_blk_gemm_nt(gmb_engine* e, double* C, int64_t ldc, const double* A, int64_t lda, const double* B,
                    int64_t ldb, int64_t m, int64_t n, int64_t k, double alpha, double beta, int32_t tri,
                    int64_t tri_shift) {
  if (!e || !C || !A || !B) return fail(e, GMB_EINVAL, "null gemm operand");
  if (m % TILE || n % TILE || k % KT || m < 0 || n < 0 || k < 0)
    return fail(e, GMB_EINVAL, "gemm sizes must be multiples of 128 (m, n) and 16 (k)");
  HIP_TRY(e, hipSetDevice(e->device));
  GemmArgs g{};
  g.C = C;
  g.ldc = ldc;
  g.A = A;
  g.lda = lda;
  g.B = B;
  g.ldb = ldb;
  g.mt = (int)(m / TILE);
  g.nt = (int)(n / TILE);
  g.k = (int)k;
  g.alpha = alpha;
  g.beta = beta;
  g.tri = tri;
  g.tri_off = (int)(tri_shift * TILE);
  return launch_gemm(e, e->stream, g, EV_CHOL_PANEL_GEMM);
}

// The same product with every field of GemmArgs and every choice of launch_gemm in the caller's hands (tests): see the header.
int gmb_blk_gemm_ex(gmb_engine* e, double* C, const double* A, const double* B, const gmb_gemm_desc* d, int32_t* launched) {
  if (launched) *launched = 0;
  if (!e) return GMB_EINVAL;
  if (!C || !A || !B || !d) return fail(e, GMB_EINVAL, "null gemm operand");
  if (d->m % TILE || d->n % TILE || d->k % KT || d->m < 0 || d->n < 0 || d->k < 0 || d->m > (1 << 24) || d->n > (1 << 24) || d->k > (1 << 24))
    return fail(e, GMB_EINVAL, "gemm sizes must be multiples of 128 (m, n) and 16 (k)");
  // the kernels move operands 16 bytes at a time
  if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)(d->lda * 8) | (uintptr_t)(d->ldb * 8)) & 15u)
    return fail(e, GMB_EINVAL, "gmb_blk_gemm_ex: A and B must be 16-byte aligned, lda and ldb even");
  if (d->nblk_stride < 0 || d->cblk_stride < 0 || d->krow_stride < 0 || d->nblk_stride > 4096 || d->cblk_stride > 4096 || d->krow_stride > 4096 ||
      (d->klo_m | d->klo_n | d->khi_n | d->tri) < 0 || (d->klo_m | d->klo_n | d->khi_n | d->tri) > 1)
    return fail(e, GMB_EINVAL, "gmb_blk_gemm_ex: strides must be >= 0, tri / klo_m / klo_n / khi_n 0 or 1");
  if (d->tri_off % 32 || d->krow_off % TILE) return fail(e, GMB_EINVAL, "gmb_blk_gemm_ex: tri_off must be a multiple of 32, krow_off of 128");
  const int64_t bs = d->nblk_stride < 1 ? 1 : d->nblk_stride, cs = d->cblk_stride > 0 ? d->cblk_stride : bs;
  const int64_t brows = d->n ? ((d->n / TILE - 1) * bs + 1) * TILE : 0, crows = d->n ? ((d->n / TILE - 1) * cs + 1) * TILE : 0;
  if (d->lda < d->m || d->ldb < brows || d->ldc < crows) return fail(e, GMB_EINVAL, "gmb_blk_gemm_ex: a leading dimension is smaller than its operand");
  if ((const double*)C == B && d->ldc != d->ldb) return fail(e, GMB_EINVAL, "gmb_blk_gemm_ex: in place needs ldc == ldb");
  if (d->variant < -1 || d->staging < -1 || d->pfc < -1 || d->order < -1 || d->strip < -1) return fail(e, GMB_EINVAL, "gmb_blk_gemm_ex: a pin below -1");
  HIP_TRY(e, hipSetDevice(e->device));
  GemmArgs g{};
  g.C = C;
  g.ldc = d->ldc;
  g.A = A;
  g.lda = d->lda;
  g.B = B;
  g.ldb = d->ldb;
  g.mt = (int)(d->m / TILE);
  g.nt = (int)(d->n / TILE);
  g.k = (int)d->k;
  g.alpha = d->alpha;
  g.beta = d->beta;
  g.tri = d->tri;
  g.tri_off = d->tri_off;
  g.nblk_stride = d->nblk_stride;
  g.cblk_stride = d->cblk_stride;
  g.klo_m = d->klo_m;
  g.klo_n = d->klo_n;
  g.khi_n = d->khi_n;
  g.krow_off = d->krow_off;
  g.krow_stride = d->krow_stride;
  GemmPin pin;
  pin.variant = d->variant;
  pin.staging = d->staging;
  pin.pfc = d->pfc;
  pin.order = d->order;
  pin.strip = d->strip;
  pin.launched = launched;
  return launch_gemm(e, e->stream, g, EV_CHOL_PANEL_GEMM, &pin);
}

// The split-k product on caller-provided blocks (tests, tools/gpu_append.py): see the header.
int gmb_blk_gemm_splitk(gmb_engine* e, double* C, int64_t ldc, const double* A, int64_t lda, const double* B, int64_t ldb, int64_t m,
                        int64_t n, int64_t k, double alpha, double beta, int32_t tri, int32_t slices, int32_t* slices_used) {
  if (slices_used) *slices_used = 0;
  if (!e) return GMB_EINVAL;
  if (!C || !A || !B) return fail(e, GMB_EINVAL, "null gemm operand");
  if (m % TILE || n % TILE || k % KT || m <= 0 || n <= 0 || k <= 0 || m > (1 << 24) || n > (1 << 24) || k > (1 << 24))
    return fail(e, GMB_EINVAL, "split-k gemm sizes must be positive multiples of 128 (m, n) and 16 (k)");
  // (the tile count is formed in 64 bits -- splitk_tile_count -- and bounded by the launch: at most 65535 computed tiles)
  if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)(lda * 8) | (uintptr_t)(ldb * 8)) & 15u)
    return fail(e, GMB_EINVAL, "gmb_blk_gemm_splitk: A and B must be 16-byte aligned, lda and ldb even");
  if (lda < m || ldb < n || ldc < n) return fail(e, GMB_EINVAL, "gmb_blk_gemm_splitk: a leading dimension is smaller than its operand");
  if (tri < 0 || tri > 1) return fail(e, GMB_EINVAL, "gmb_blk_gemm_splitk: tri must be 0 or 1");
  if (slices != -1 && slices < 1) return fail(e, GMB_EINVAL, "gmb_blk_gemm_splitk: slices must be -1 (by the rule) or >= 1");
  HIP_TRY(e, hipSetDevice(e->device));
  SplitKArgs a{};
  a.C = C;
  a.ldc = ldc;
  a.A = A;
  a.lda = lda;
  a.B = B;
  a.ldb = ldb;
  a.mt = (int)(m / TILE);
  a.nt = (int)(n / TILE);
  a.k = (int)k;
  a.alpha = alpha;
  a.beta = beta;
  a.tri = tri;
  return launch_gemm_splitk(e, e->stream, a, slices, slices_used);
}

int gmb_append(gmb_engine* e, const double* Xnew, int64_t K, int64_t ldx, const double* ynew, int32_t memspace) {
  int rc = resize_ready(e, "gmb_append");
  if (rc) return rc;
  if (!Xnew || !ynew || K < 0 || ldx < e->D) return fail(e, GMB_EINVAL, "gmb_append: bad Xnew/K/ldx/ynew");
  if (K == 0) return GMB_OK;
  return resize_n(e, e->N + K, Xnew, K, ldx, ynew, memspace, "gmb_append");
}

int64_t gmb_num_obs(const gmb_engine* e) { return e ? e->N : (int64_t)GMB_EINVAL; }

int gmb_truncate(gmb_engine* e, int64_t n_keep) {
  int rc = resize_ready(e, "gmb_truncate");
  if (rc) return rc;
  if (n_keep < 1 || n_keep > e->N) return fail(e, GMB_EINVAL, "gmb_truncate: n_keep = %lld must be in [1, %lld]", (long long)n_keep, (long long)e->N);
  if (n_keep == e->N) return GMB_OK;
  return resize_n(e, n_keep, nullptr, 0, 0, nullptr, GMB_HOST, "gmb_truncate");
}

}  // extern "C"

#include "dist_driver.hpp"
#include "dist_capacity.hpp"

extern "C" {

// 0 = replicated factor (default: every rank ends with the complete factor), 1 = capacity (dist_capacity.hpp: owned block rows
// + panel buffers only).  Takes effect with the next gmb_dist_factorize; returns the previous mode or a negative status.
int gmb_dist_set_mode(gmb_engine* e, int32_t mode) {
  if (!e || mode < 0 || mode > 1) return GMB_EINVAL;
  const int old = e->dist_mode;
  if (old != mode) e->fs.inputs_changed();
  e->dist_mode = mode;
  // the point of mode 1 is that no rank keeps an Nr x Np buffer: one left behind by an earlier single-engine or replicated
  // factorisation goes now (its factorisation was just invalidated, or is of no use to the capacity passes)
  if (mode == 1 && e->dA && e->dA.cap > 0) {
    if (hipSetDevice(e->device) == hipSuccess) (void)hipStreamSynchronize(e->stream);
    e->dA.drop(e->pool);
    e->fs.inputs_changed();
  }
  return old;
}

// device bytes this engine holds through its own allocations right now (peak != 0: the largest value so far)
int64_t gmb_resident_bytes(const gmb_engine* e, int32_t peak) {
  if (!e) return GMB_EINVAL;
  return peak ? e->pool.bytes_peak : e->pool.bytes_resident;
}

int gmb_dist_factorize(gmb_engine* e, const gmb_comm* comm, int32_t panel_blocks) {
  if (!e) return GMB_EINVAL;
  if (e->periodic) return fail(e, GMB_EINVAL, "gmb_dist_factorize: periodic kernels are not supported by the multi-GPU driver");
  return e->dist_mode == 1 ? cap_factorize(e, comm, panel_blocks) : dist_factorize(e, comm, panel_blocks);
}

int gmb_dist_nlml(gmb_engine* e, const gmb_comm* comm, double* nlml, double* grad) {
  if (!e) return GMB_EINVAL;
  return e->dist_mode == 1 ? cap_nlml(e, comm, nlml, grad) : dist_nlml(e, comm, nlml, grad);
}

int gmb_dist_predict(gmb_engine* e, const gmb_comm* comm, const double* Xs, int64_t M, int64_t ldxs, int32_t with_noise,
                     double* mean, double* var, int32_t memspace) {
  if (!e) return GMB_EINVAL;
  return e->dist_mode == 1 ? cap_predict(e, comm, Xs, M, ldxs, with_noise, mean, var, memspace)
                           : dist_predict(e, comm, Xs, M, ldxs, with_noise, mean, var, memspace);
}

}  // extern "C"
