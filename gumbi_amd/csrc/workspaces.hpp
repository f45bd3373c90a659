// workspaces.hpp -- the engine's workspaces, and what each guarded call asks of them.
//
// A workspace is a row group (device_buffers.hpp).  Each struct writes its members ONCE, in each(): (buffer, element count) pairs
// for a row count and its other size arguments.  reserve() renews by walking that list, bytes() sums sizeof(T) * count over it and
// a Budget measures with the two, so what a call is refused for and what it allocates cannot drift apart.  The counts are
// doubles: a request that has to be refused may not fit in int64_t, and every count that IS allocated is an integer below 2^53.
// One level up, predict_buffers / joint_buffers / group_buffers / design_buffers / batch_buffers / paths_*_buffers list every buffer of a call once, over a visitor
// (a Budget, then a Reserver); they are templates over the engine, of which they use N, Np, D and the members named in them.
//
// No HIP and no engine types: tools/workspace_budget_check.cpp runs this very header over a host allocator.
#pragma once
#include "batch_plan.hpp"
#include "design_plan.hpp"
#include "device_buffers.hpp"
#include "fitc_plan.hpp"
#include "laplace_plan.hpp"
#include "paths_plan.hpp"
#include "slope_plan.hpp"  // SLOPE_MAX_COLS
#include "workspace_sizes.hpp"

namespace gmb {

// what every workspace derives from its list: Self::each(rows, <size arguments>, f) calls f(buffer, element count) for every member
// while f says "go on".  A workspace whose SHAPE can grow (more entries per row, a further member) hides held() and sized_for():
// it holds no rows for a larger shape, and is renewed whole for one.
template <class Self>
struct Workspace : RowGroup {
  template <typename... Args>
  double bytes(double n, Args... args) {
    double sum = 0.0;
    self().each(n, args..., [&](auto& b, double count) { return sum += sizeof(*b.p) * count, true; });
    return sum;
  }
  template <typename... Args>  // rows that serve a request with these size arguments
  int64_t held(Args...) const { return rows; }
  template <typename... Args>  // the members were renewed for these
  void sized_for(Args...) {}
  template <typename... Args>
  int reserve(DevPool& pool, int64_t n, Args... args) {
    if (!self().held(args...)) stale();
    return reserve_rows(n, [&] {
      int rc = 0;
      self().each((double)n, args..., [&](auto& b, double count) { return !(rc = b.renew(pool, (int64_t)count)); });
      if (!rc) self().sized_for(args...);
      return rc;
    });
  }
  Self& self() { return *static_cast<Self*>(this); }
};

struct PreparedPoints : Workspace<PreparedPoints> {  // the training points as the covariance kernels read them (SoA, stride = rows)
  DevBuf<double> xs, xl;
  DevBuf<int32_t> cat;
  template <class F>
  bool each(double n, F&& f) { return f(xs, XS_ROWS * n) && f(xl, MAX_LIN * n) && f(cat, MAX_TABS * n); }
};

struct PredictWorkspace : Workspace<PredictWorkspace> {  // what an M-tile of Mt rows of a prediction needs
  DevBuf<double> dV, dXs, txs, txl;
  DevBuf<int32_t> tcat;
  DevBuf<double> dkss, dmean, dvar;
  template <class F>
  bool each(double Mt, int64_t Np, int D, F&& f) {
    return f(dV, Mt * (double)Np) && f(dXs, Mt * D) && f(txs, XS_ROWS * Mt) && f(txl, MAX_LIN * Mt) && f(tcat, MAX_TABS * Mt) && f(dkss, Mt) &&
           f(dmean, Mt) && f(dvar, Mt);
  }
};

struct GemmFormWorkspace : Workspace<GemmFormWorkspace> {  // the product form's second V (predict_form.hpp)
  DevBuf<double> dV2;  // Np x Mt: the solved cross-covariance with the TRAINING index fastest
  template <class F>
  bool each(double Mt, int64_t Np, F&& f) { return f(dV2, Mt * (double)Np); }
};

struct PredictGradWorkspace : Workspace<PredictGradWorkspace> {  // gmb_predict_grad's own, beside a prediction's (predict_grad.hpp)
  DevBuf<double> Xs, xs, xl;
  DevBuf<int32_t> cat;
  DevBuf<double> grad;
  template <class F>
  bool each(double Mt, int D, F&& f) { return f(Xs, Mt * D) && f(xs, XS_ROWS * Mt) && f(xl, MAX_LIN * Mt) && f(cat, MAX_TABS * Mt) && f(grad, Mt * D); }
};

// gmb_predict_decompose (predict_terms.hpp): the chunked partials of an M-tile ([chunk][entry][Mt], `entries` = chunks x entries)
// and its results (T means, T (T + 1) / 2 covariance rows, the noise: rows of Mt)
struct TermsWorkspace : Workspace<TermsWorkspace> {
  DevBuf<double> part, out;
  int64_t per_row = 0;  // the entries the rows were sized for
  template <class F>
  bool each(double Mt, int64_t entries, F&& f) { return f(part, (double)entries * Mt) && f(out, (tg_entries(TG_MAX_TERMS) + 1) * Mt); }
  int64_t held(int64_t entries) const { return per_row < entries ? 0 : rows; }
  void sized_for(int64_t entries) { per_row = entries; }
};

// gmb_predict_groups (group_average.hpp), sized by the call's M points and by nothing of size M x N: the raw and the prepared
// points, their weights and one row block of R (128 x M)
struct GroupWorkspace : Workspace<GroupWorkspace> {
  DevBuf<double> Xs, xs, xl, w, R;
  DevBuf<int32_t> cat;
  template <class F>
  bool each(double Mp, int D, F&& f) {
    return f(Xs, Mp * D) && f(xs, XS_ROWS * Mp) && f(xl, MAX_LIN * Mp) && f(w, Mp) && f(R, GA_ROWS * Mp) && f(cat, MAX_TABS * Mp);
  }
};

// gmb_predict_slope (predict_slope.hpp): the chunked partials of an M-tile ([chunk][entry][Mt]), the prior curvature (Dc rows of
// Mt) and the results in the caller's layout (Mt x D twice, Mt x D x D when the covariance is asked for)
struct SlopeWorkspace : Workspace<SlopeWorkspace> {
  DevBuf<double> part, prior, mean, var, cov;
  int64_t per_row = 0;  // the entries the partials were sized for
  bool has_cov = false;
  template <class F>
  bool each(double Mt, int64_t entries, int D, bool with_cov, F&& f) {
    return f(part, (double)entries * Mt) && f(prior, SLOPE_MAX_COLS * Mt) && f(mean, Mt * D) && f(var, Mt * D) && (!with_cov || f(cov, Mt * D * D));
  }
  int64_t held(int64_t entries, int, bool with_cov) const { return per_row < entries || (with_cov && !has_cov) ? 0 : rows; }
  void sized_for(int64_t entries, int, bool with_cov) { per_row = entries, has_cov = with_cov; }
};

// gmb_design_batch (design_batch.hpp), by the Mc padded candidates of a DesignPlan: the candidates raw and prepared, their solved
// rows dVc (Mc x Np), D (Mc rows of ld), the pick's row, the weights and latent variances by column of D, the step kernel's
// partial sums ([chunk][Mc]), noise and mask by candidate, the control block and the results' staging (`res` doubles)
struct DesignWorkspace : Workspace<DesignWorkspace> {
  DevBuf<double> Xs, xs, xl, dVc, dD, dpiv, w, var, part, noise, ctl, res;
  DevBuf<int32_t> cat, mask;
  int64_t for_np = 0, for_ld = 0, for_chunks = 0, for_res = 0;
  int for_d = 0;
  template <class F>
  bool each(double Mc, int64_t Np, int64_t ld, int64_t nchunk, int64_t nres, int D, F&& f) {
    return f(Xs, Mc * D) && f(xs, XS_ROWS * Mc) && f(xl, MAX_LIN * Mc) && f(cat, MAX_TABS * Mc) && f(dVc, Mc * (double)Np) &&
           f(dD, Mc * (double)ld) && f(dpiv, (double)ld) && f(w, (double)ld) && f(var, (double)ld) && f(part, (double)nchunk * Mc) &&
           f(noise, Mc) && f(mask, Mc) && f(ctl, (double)DesignPlan::DESIGN_CTL_DOUBLES) && f(res, (double)nres);
  }
  int64_t held(int64_t Np, int64_t ld, int64_t nchunk, int64_t nres, int D) const {
    return for_np < Np || for_ld < ld || for_chunks < nchunk || for_res < nres || for_d < D ? 0 : rows;
  }
  void sized_for(int64_t Np, int64_t ld, int64_t nchunk, int64_t nres, int D) {
    for_np = Np, for_ld = ld, for_chunks = nchunk, for_res = nres, for_d = D;
  }
};

// gmb_predict_batches (predict_batches.hpp), by the batches of its largest M-tile: the chunked partial tiles (`part` doubles: the
// plan's slots x accumulators x q x q), the covariance blocks (q x q per batch) and, with gradients, their derivatives (x D)
struct BatchWorkspace : Workspace<BatchWorkspace> {
  DevBuf<double> part, cov, dcov;
  double for_part = 0.0;
  int for_q = 0, for_d = 0;
  bool has_grad = false;
  template <class F>
  bool each(double nb, double npart, int q, int D, bool grad, F&& f) {
    return f(part, npart) && f(cov, nb * q * q) && (!grad || f(dcov, nb * q * q * D));
  }
  int64_t held(double npart, int q, int D, bool grad) const {
    return for_part < npart || for_q < q || for_d < D || (grad && !has_grad) ? 0 : rows;
  }
  void sized_for(double npart, int q, int D, bool grad) { for_part = npart, for_q = q, for_d = D, has_grad = grad; }
};

// The pathwise posterior draws (pathwise.hpp): what gmb_paths_prepare leaves resident -- A = Sigma^-1 R and the scaled
// feature weights, both draw-fastest ([index][Sp]), the frequencies by prepared column and the phases -- and the calls' own
// buffers: the results of one M-tile ([draw][point]), the chunked partials, the own-draw values and draw indices, the staged
// normals of a preparation.  `epoch` is FactorState's when the state was prepared: a state of another epoch is stale.
struct PathState {
  bool ready = false;
  unsigned epoch = 0;
  int32_t S = 0, Sp = 0;
  int64_t F = 0, F4 = 0;
  DevBuf<double> A, wt, omega, phase;
  DevBuf<double> out, part, val, eps;
  DevBuf<int32_t> draw;
  void clear() { ready = false, S = Sp = 0, F = F4 = 0; }
};

// The sparse (FITC) path (fitc.hpp).  Two m x tile blocks with the tile's columns fastest (what the cross-covariance
// launch writes and the triangular solves work on) ...
struct FitcSolveWorkspace : Workspace<FitcSolveWorkspace> {
  DevBuf<double> V1, V2;
  int64_t for_mp = 0;
  template <class F>
  bool each(double rows, int64_t mp, F&& f) { return f(V1, rows * (double)mp) && f(V2, rows * (double)mp); }
  int64_t held(int64_t mp) const { return for_mp < mp ? 0 : rows; }
  void sized_for(int64_t mp) { for_mp = mp; }
};
// ... two with the inducing index fastest (the GEMMs' operands: leading dimension mr, the border row included) ...
struct FitcGemmWorkspace : Workspace<FitcGemmWorkspace> {
  DevBuf<double> S1, S2;
  int64_t for_mr = 0;
  template <class F>
  bool each(double rows, int64_t mr, F&& f) { return f(S1, rows * (double)mr) && f(S2, rows * (double)mr); }
  int64_t held(int64_t mr) const { return for_mr < mr ? 0 : rows; }
  void sized_for(int64_t mr) { for_mr = mr; }
};
// ... and the test points of one M-tile of gmb_fitc_predict, raw and prepared, with their results
struct FitcTestPoints : Workspace<FitcTestPoints> {
  DevBuf<double> Xs, xs, xl;
  DevBuf<int32_t> cat;
  DevBuf<double> kss, mean, var;
  template <class F>
  bool each(double Mt, int D, F&& f) {
    return f(Xs, Mt * D) && f(xs, XS_ROWS * Mt) && f(xl, MAX_LIN * Mt) && f(cat, MAX_TABS * Mt) && f(kss, Mt) && f(mean, Mt) && f(var, Mt);
  }
};

// Everything the sparse path keeps on the device.  Nothing here has N x N elements, and none of the exact path's buffers is used.
struct FitcState {
  int64_t m = 0, mp = 0, mr = 0;  // inducing points; padded; rows of the bordered layout
  bool have_z = false;            // gmb_fitc_set_inducing succeeded for the current data and kernel
  bool resident = false;          // Lu, L_B, c and w belong to the current (data, Z, theta): gmb_fitc_predict may run
  DevBuf<double> dZ;              // m x D, row-major: the inducing points as handed in
  PreparedPoints zpts;            // ... as the covariance kernels read them (stride mr)
  DevBuf<double> dKuu, dB;        // mr x mp, bordered layout: Kuu then Lu; B then L_B with c = L_B^-1 A Lambda^-1 y in row m
  DevBuf<double> dP;              // mp x mp: sum over the tiles of G_uf A^T, then G_uu (without its -1/2)
  DevBuf<double> dDinvU, dDinvB;  // sub-block inverses of the two factors' diagonal blocks
  DevBuf<double> dscalU, dscalB;  // their scalar blocks: [0] log-det, the info word at SCAL_INFO_AT
  DevBuf<uint32_t> dctU, dctB;    // control blocks of the persistent tile kernel
  DevBuf<double> dzero;           // mr zeros: Kuu's border row
  DevBuf<double> dcw;             // 3 mp: c | w = L_B^-T c | the back substitution's running right-hand side
  DevBuf<double> dlam, dalpha, dd;  // Np each: lambda, alpha, d
  DevBuf<double> dcolpart;        // [block of 32 columns][FITC_COL_SUMS]
  DevBuf<double> dredpart;        // [workgroup][FITC_DERIV_SUMS] of one derivative reduction
  DevBuf<double> dacc;            // FITC_ACC_DOUBLES: the folded sums (fitc.hpp)
  FitcSolveWorkspace sw;
  FitcGemmWorkspace gw;
  FitcTestPoints tp;
  void drop_inducing() { have_z = resident = false, m = mp = mr = 0; }
};
constexpr int FITC_ACC_DOUBLES = 64;  // [0] sum log lambda [1] sum y^2 / lambda [2] sum d | [8, 25) G_uf's sums | [32, 49) G_uu's

// GP classification by the Laplace approximation (laplace.hpp): what it keeps beside the exact path's factor buffer
// (B, then its factor) and inverse buffer (B^-1, then Z').  dS is the one N x N matrix of its own, allocated only by these calls.
struct LaplaceState {
  bool resident = false;   // the mode, s, g and B's factor in the factor buffer belong to the current (data, labels, kernel, theta)
  const char* dropped_by = "no gmb_laplace_evaluate has succeeded";  // ... or what took them away
  double tol = 1e-9;       // gmb_laplace_set_options
  int32_t max_iter = 40;
  int32_t iterations = 0, halvings = 0;  // of the last evaluation (gmb_laplace_info)
  double psi = 0.0, step = 0.0;
  bool f_swapped = false;  // which of the two f vectors holds the mode (they change roles when a step is accepted)
  DevBuf<double> dS;       // Sigma: Nr x Np, the bordered layout of the factor buffer (the covariance build writes it)
  DevBuf<double> dvec;     // LAP_VECTORS vectors of Np
  DevBuf<double> dsymv;    // the slots of symv_lower_kernel
  DevBuf<double> dlikpart; // the partial sets of laplace_lik_kernel
  DevBuf<double> dsums;    // LAP_LIK_SUMS: their fold
  void drop(const char* why) {
    if (resident) dropped_by = why;
    resident = false;
  }
};
// the vectors of dvec
enum LapVec : int {
  LV_F0 = 0, LV_F1, LV_A, LV_AC, LV_AH, LV_PI, LV_W, LV_S, LV_G, LV_B, LV_T1, LV_T2, LV_T3, LV_S2, LV_U, LV_SPARE
};
static_assert(LV_SPARE + 1 == LAP_VECTORS, "laplace_plan.hpp counts the vectors");

// ---- what a call asks for: its buffers, listed once (`v`: a Budget or a Reserver) ---------------------------------------------------

// the sparse path, in three lists: what depends on m alone (gmb_fitc_set_inducing allocates it) ...
template <class V>
bool fitc_fixed_buffers(FitcState& s, const FitcPlan& pl, int D, V& v) {
  const double mp = (double)pl.mp, mr = (double)pl.mr, nb = mp / FITC_TILE;
  return v.buf(s.dZ, (double)pl.m * D) && v.rows(s.zpts, mr) && v.buf(s.dKuu, mr * mp) && v.buf(s.dB, mr * mp) && v.buf(s.dP, mp * mp) &&
         v.buf(s.dDinvU, nb * 8 * 256) && v.buf(s.dDinvB, nb * 8 * 256) && v.buf(s.dscalU, 72.0) && v.buf(s.dscalB, 72.0) && v.buf(s.dzero, mr) &&
         v.buf(s.dcw, 3.0 * mp) && v.buf(s.dacc, (double)FITC_ACC_DOUBLES);
}
// ... the m x tile blocks of `rows` columns (an evaluation: the widest tile of X; a prediction: its M-tile, without the GEMM operands) ...
template <class V>
bool fitc_block_buffers(FitcState& s, const FitcPlan& pl, double rows, bool gemm_operands, V& v) {
  return v.rows(s.sw, rows, pl.mp) && (!gemm_operands || (v.rows(s.gw, rows, pl.mr) && v.buf(s.dredpart, (double)pl.deriv_blocks() * FITC_DERIV_SUMS)));
}
// ... and the per-column vectors of an evaluation: O(N)
template <class V>
bool fitc_column_buffers(FitcState& s, const FitcPlan& pl, V& v) {
  return v.buf(s.dlam, (double)pl.Np) && v.buf(s.dalpha, (double)pl.Np) && v.buf(s.dd, (double)pl.Np) &&
         v.buf(s.dcolpart, (double)pl.col_blocks() * FITC_COL_SUMS);
}
template <class V>
bool fitc_evaluate_buffers(FitcState& s, const FitcPlan& pl, int D, V& v) {
  return fitc_fixed_buffers(s, pl, D, v) && fitc_block_buffers(s, pl, (double)pl.tmax, true, v) && fitc_column_buffers(s, pl, v);
}
template <class V>
bool fitc_predict_buffers(FitcState& s, const FitcPlan& pl, double Mt, int D, V& v) {
  return fitc_block_buffers(s, pl, Mt, false, v) && v.rows(s.tp, Mt, D);
}

// the Laplace path: everything of an evaluation that is its own (the factor buffer, the inverse's and the gradient's vectors are the
// exact path's and sized by it; a prediction adds predict_buffers alone)
template <class V>
bool laplace_evaluate_buffers(LaplaceState& s, const LaplacePlan& pl, V& v) {
  return v.buf(s.dS, pl.sigma_doubles()) && v.buf(s.dvec, pl.vector_doubles()) && v.buf(s.dsymv, pl.symv_doubles()) &&
         v.buf(s.dlikpart, pl.lik_doubles()) && v.buf(s.dsums, (double)LAP_LIK_SUMS);
}
// chunks of the posterior reductions' first stage over the N training rows
inline int red_chunks(int64_t N) { return (int)((N + RED_CHUNK - 1) / RED_CHUNK); }

// a prediction's M-tiles of Mt rows: the workspace and the two chunked partial sums (mean, variance) of a tile
template <class E, class V>
bool predict_buffers(E& e, double Mt, V& v) {
  return v.rows(e.pw, Mt, e.Np, e.D) && v.buf(e.dpart, 2.0 * red_chunks(e.N) * Mt);
}

// elements of the joint posterior's second matrix (bordered layout: Mr = M + 1 rounded up to a tile, Mp = M rounded up)
inline double joint_matrix_elems(double Mr, double Mp) { return Mr * Mp; }

// a joint posterior: V whole (all Mr rows in ONE tile), the product form's second V, C, and `stage` doubles of device staging
template <class E, class V>
bool joint_buffers(E& e, double Mr, double Mp, bool gemm_form, double stage, V& v) {
  return predict_buffers(e, Mr, v) && (!gemm_form || v.rows(e.pw2, Mr, e.Np)) && v.buf(e.jt.dC, joint_matrix_elems(Mr, Mp)) &&
         (stage <= 0.0 || v.buf(e.jt.dstage, stage));
}

// elements of the task partials of one reduction of gmb_predict_groups ([task][column]): all tasks against the training points, or
// the fullest row block's against the call's own
inline double group_partial_elems(double ntask, double block_tasks, double Np, double Mp) {
  return ntask * Np > block_tasks * Mp ? ntask * Np : block_tasks * Mp;
}

// gmb_predict_groups: a prediction's buffers for Gr = G + 1 rounded up rows (NEVER for M) -- a joint posterior's when the covariance
// is asked for -- then the feature's own workspace for Mp rows, the task partials and the index arrays (the task triples, then
// first_task and offsets: G + 1 each)
template <class E, class V>
bool group_buffers(E& e, double Mp, double G, double Gr, double Gp, double ntask, double block_tasks, bool gemm_form, bool with_cov,
                   double stage, V& v) {
  return (with_cov ? joint_buffers(e, Gr, Gp, gemm_form, stage, v) : predict_buffers(e, Gr, v) && (!gemm_form || v.rows(e.pw2, Gr, e.Np))) &&
         v.rows(e.ga, Mp, e.D) && v.buf(e.ga_part, group_partial_elems(ntask, block_tasks, (double)e.Np, Mp)) &&
         v.buf(e.ga_idx, 3.0 * ntask + 2.0 * (G + 1.0));
}

// gmb_design_batch: a prediction's buffers for the plan's largest point tile (`mt` rows, NEVER all M + R), the product form's
// second V, then the feature's own workspace (`nres`: doubles of the results' staging)
template <class E, class V>
bool design_buffers(E& e, const DesignPlan& pl, double nres, bool gemm_form, V& v) {
  return predict_buffers(e, (double)pl.mt, v) && (!gemm_form || v.rows(e.pw2, (double)pl.mt, e.Np)) &&
         v.rows(e.dz, (double)pl.Mc, e.Np, pl.ld, pl.nchunk, (int64_t)nres, (int)e.D);
}

// gmb_predict_batches: a prediction's buffers for the plan's largest tile, the feature's own workspace for `nacc` accumulators per
// (chunk, batch) and, with gradients, gmb_predict_grad's workspace for the same tile (`pg_part`: doubles of its partials)
template <class E, class V>
bool batch_buffers(E& e, const BatchPlan& pl, int nacc, bool grad, double pg_part, V& v) {
  return predict_buffers(e, (double)pl.mt, v) && v.rows(e.bw, pl.cov_doubles() / (pl.q * pl.q), pl.part_doubles(nacc), (int)pl.q, (int)e.D, grad) &&
         (!grad || (v.rows(e.pg, (double)pl.mt, (int)e.D) && v.buf(e.pg_part, pg_part)));
}

// gmb_paths_prepare: a prediction's buffers for `mrow` rows (the draws as test index), the resident state, the staged normals
// (S x N) and the feature pass over the training points (`pl`: the features-only plan at M = N)
template <class E, class V>
bool paths_prepare_buffers(E& e, PathState& st, const PathsPlan& pl, double mrow, V& v) {
  return predict_buffers(e, mrow, v) && v.buf(st.A, (double)e.Np * pl.Sp) && v.buf(st.wt, (double)pl.F4 * pl.Sp) &&
         v.buf(st.omega, (double)e.nc_pad * (double)pl.F4) && v.buf(st.phase, (double)pl.F4) && v.buf(st.eps, (double)pl.S * (double)e.N) &&
         v.buf(st.out, pl.out_doubles()) && v.buf(st.part, pl.part_doubles());
}
// gmb_paths_eval: the points of the largest M-tile raw and prepared (gmb_predict_grad's workspace), its results and partials
template <class E, class V>
bool paths_eval_buffers(E& e, PathState& st, const PathsPlan& pl, V& v) {
  return v.rows(e.pg, (double)pl.mt, (int)e.D) && v.buf(st.out, pl.out_doubles()) && v.buf(st.part, pl.part_doubles());
}
// gmb_paths_eval_own: the same points, the values, the draw indices and the partials of nc_pad + 1 accumulators
template <class E, class V>
bool paths_own_buffers(E& e, PathState& st, const PathsPlan& pl, V& v) {
  return v.rows(e.pg, (double)pl.mt, (int)e.D) && v.buf(st.val, (double)pl.mt) && v.buf(st.draw, (double)pl.mt) &&
         v.buf(st.part, pl.own_part_doubles(e.nc_pad + 1));
}

}  // namespace gmb
