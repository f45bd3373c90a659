// factor_state_check.cpp -- gumbi_amd/csrc/factor_state.hpp (the very header engine.hip keeps its validity marks in) against a
// frozen copy of the seven loose fields and the hand-written assignments it replaced, as a stand-alone program for the
// sanitizers.  No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/factor_state_check.cpp -o /tmp/factor_state_check
//   /tmp/factor_state_check
//
// The ABI is modelled as EVENTS: an entry point together with one of its outcomes (gmb_factorize: accepted / not positive
// definite / abandoned and retried ...).  Every event is written down twice:
//   * old_event: the assignments of engine.hip, dist_driver.hpp and dist_capacity.hpp as they stood at commit 4f7a785, verbatim,
//     on a verbatim copy of the seven fields (`Old`: THE ORACLE -- frozen, never edited to follow the engine; the line numbers in
//     its comments are that commit's);
//   * new_event: the transitions the same entry point performs today, transcribed from the functions named in the comments.
// Both carry the little of the engine the guards look at beside the marks (is there data, a kernel, a theta, a factor buffer, the
// capacity driver's rows; the distribution mode) and decide themselves whether a guard refuses -- a refused event changes nothing.
//
// Every sequence of up to MAX_EVENTS events is replayed from a freshly created engine through both (a state that has been
// expanded with as many events to go is not expanded again: equal states have equal futures).  After every event all seven
// values must be equal, the rest of the engine must be equal, and every predicate must return what the old spelled-out
// expression returns.  The first difference prints its sequence and ends the program with status 1
// (tests/test_factor_state_cpu.py builds and runs it without the sanitizers).
//
// A new mark: one field and its transitions in the header, its value in `same()`, and its assignments -- as the entry points make
// them the day it is added -- in the oracle.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../gumbi_amd/csrc/factor_state.hpp"

using gmb::FactorState;

// what the guards read beside the marks
struct Rest {
  bool data = false, spec = false, theta = false;  // N > 0, have_spec, have_theta
  int dist_mode = 0;
  bool dA = false, dAown = false;  // a factor buffer is allocated; the capacity driver's own rows are
  bool operator==(const Rest& o) const {
    return data == o.data && spec == o.spec && theta == o.theta && dist_mode == o.dist_mode && dA == o.dA && dAown == o.dAown;
  }
};

// five events needs three of them to make an engine ready (data, kernel, theta); eight = those three and five more
constexpr int MAX_EVENTS = 8;

enum Event {
  SET_DATA, SET_DATA_LARGER, SET_Y, SET_KERNEL, SET_PERIODIC, SET_THETA,
  FACTORIZE_OK, FACTORIZE_NOTPD, FACTORIZE_ABANDONED_RETRY_OK, FACTORIZE_ABANDONED_RETRY_FAILS, FACTORIZE_NO_BUFFER,
  EVALUATE_OK, EVALUATE_NOTPD,
  EVALUATE_GRAD_FUSED_OK, EVALUATE_GRAD_FUSED_FINISH_FAILS, EVALUATE_GRAD_FUSED_GRADIENT_FAILS, EVALUATE_GRAD_FUSED_ABANDONED_RETRY_OK,
  EVALUATE_GRAD_TILES_OK, EVALUATE_GRAD_TREE_OK, EVALUATE_GRAD_TREE_FAILS_MIDWAY, EVALUATE_GRAD_TREE_FAILS_MIDWAY_NOTPD,
  NLML_GRAD_TILES_OK, NLML_GRAD_TILES_ABANDONED, NLML_GRAD_TREE_OK, NLML_GRAD_TREE_FAILS_MIDWAY,
  PREDICT, PREDICT_JOINT, PREDICT_GRAD,
  RESIZE_OK, RESIZE_OK_BUFFER_TOO_SMALL, RESIZE_BAIL, RESIZE_TAIL_FAILS,
  DIST_SET_MODE_0, DIST_SET_MODE_1,
  DIST_FACTORIZE_OK, DIST_FACTORIZE_FAILS, DIST_NLML_GRAD_OK, DIST_NLML_GRAD_FAILS,
  DEBUG_ASSUME_FACTORED,
  N_EVENTS
};

static const char* const EVENT_NAMES[N_EVENTS] = {
  "set_data", "set_data(larger)", "set_y", "set_kernel", "set_periodic", "set_theta",
  "factorize:ok", "factorize:notpd", "factorize:abandoned,retry-ok", "factorize:abandoned,retry-fails", "factorize:no-buffer",
  "evaluate:ok", "evaluate:notpd",
  "evaluate(grad):fused,ok", "evaluate(grad):fused,finish-fails", "evaluate(grad):fused,gradient-fails",
  "evaluate(grad):fused,abandoned,retry-ok",
  "evaluate(grad):tiles,ok", "evaluate(grad):tree,ok", "evaluate(grad):tree,fails-midway", "evaluate(grad):tree,fails-midway,notpd",
  "nlml(grad):tiles,ok", "nlml(grad):tiles,abandoned", "nlml(grad):tree,ok", "nlml(grad):tree,fails-midway",
  "predict", "predict_joint", "predict_grad",
  "resize:ok", "resize:ok,buffer-too-small", "resize:bail", "resize:tail-fails",
  "dist_set_mode(0)", "dist_set_mode(1)",
  "dist_factorize:ok", "dist_factorize:fails", "dist_nlml(grad):ok", "dist_nlml(grad):fails",
  "debug_assume_factored",
};

// =====================================================================================================================================
// THE ORACLE: the fields of gmb_engine (engine.hip:172-178, 203, 232 at 4f7a785) and every assignment to them.  Frozen.
// =====================================================================================================================================
struct Old {
  bool factored = false;
  enum { FK_NONE = 0, FK_SINGLE = 1, FK_REPLICATED = 2, FK_CAPACITY = 3 };
  int factor_kind = FK_NONE;
  bool factor_consumed = false;
  bool have_alpha = false;
  bool u_valid = false, linv_valid = false;
  bool bs_valid = false;
  Rest r;
};

namespace old_engine {

// require_ready (2262-2270)
bool require_ready(const Old* e, bool need_factor) {
  if (!e->r.data || !e->r.spec || !e->r.theta) return false;
  if (need_factor && !e->factored) return false;
  return true;
}
// require_full_factor (2275-2280), require_capacity_factor (2282-2287)
bool require_full_factor(const Old* e) { return !(e->factor_kind == Old::FK_CAPACITY || !e->r.dA); }
bool require_capacity_factor(const Old* e) { return !(e->factor_kind != Old::FK_CAPACITY || !e->r.dAown); }
// gmb_factor_valid (2665)
bool factor_valid(const Old* e) { return e->r.data && e->r.theta && e->factored && !e->factor_consumed; }
// has_live_factor (2896-2898)
bool has_live_factor(const Old* e) { return e->factored && e->factor_kind == Old::FK_SINGLE && !e->factor_consumed && e->r.dA; }
// resize_ready (2901-2909)
bool resize_ready(const Old* e) {
  if (!require_ready(e, false)) return false;
  if (e->r.dist_mode != 0 || e->factor_kind == Old::FK_REPLICATED || e->factor_kind == Old::FK_CAPACITY) return false;
  if (e->factored && e->factor_consumed) return false;
  return true;
}
// predict_takes_gemm_form (3116-3119), the workspaces granted
bool predict_takes_gemm_form(const Old* e) { return e->u_valid && e->have_alpha && e->factor_kind == Old::FK_SINGLE; }
// joint_ready (3251-3259)
bool joint_ready(const Old* e) {
  if (!require_ready(e, true)) return false;
  if (e->r.dist_mode != 0 || e->factor_kind != Old::FK_SINGLE) return false;
  if (!require_full_factor(e)) return false;
  if (e->factor_consumed) return false;
  return true;
}
// predict_sel without a selection and without the capacity driver's hook (3686-3698)
bool predict_ready(const Old* e) {
  if (!require_ready(e, true)) return false;
  if (!require_full_factor(e)) return false;
  if (e->factor_consumed) return false;
  return true;
}
// gmb_copy_factor's first test (3977), gmb_copy_alpha's (4002), the debug door's (4221)
bool copy_factor_refuses(const Old* e) { return e->factored && !require_full_factor(e); }
bool copy_alpha_ready(const Old* e) { return require_ready(e, false) && e->have_alpha; }
bool door_opens(const Old* e) { return !(e->factor_kind == Old::FK_NONE || !e->r.theta); }

// gmb_set_theta (2599-2631), its guards passed
void set_theta(Old* e) {
  e->factored = false;
  e->bs_valid = false;
  e->factor_kind = Old::FK_NONE;
  e->r.theta = true;
}
// factorize_enqueue (2671-2749); `buffer`: ensure_factor_buffer succeeds; `fused`: eval_tiles rides along (2720 -> 1377)
bool factorize_enqueue(Old* e, bool buffer, bool fused) {
  e->factored = false;
  e->factor_kind = Old::FK_SINGLE;
  e->factor_consumed = false;
  e->have_alpha = false;
  e->bs_valid = false;
  e->u_valid = e->linv_valid = false;
  if (!buffer) return false;
  e->r.dA = true;
  if (fused) e->u_valid = e->linv_valid = false;  // eval_tiles, 1377
  return true;
}
// factorize_finish (2752-2786)
bool factorize_finish(Old* e, bool ok) {
  e->factored = false;
  if (!ok) return false;
  e->factored = true;
  return true;
}
enum Grad { TILES_FUSED_OK, TILES_FUSED_FAILS, TILES_OK, TILES_ABANDONED, TREE_OK, TREE_FAILS_MIDWAY };
// grad_accumulate (2071-2173) behind its own guard (2073)
bool grad_accumulate(Old* e, Grad g) {
  if (e->factor_consumed) return false;
  switch (g) {
    case TILES_FUSED_FAILS: return false;  // (an error before anything is marked)
    case TILES_FUSED_OK:                   // the light path, 2111-2113
      e->have_alpha = true;
      e->u_valid = true;
      return true;
    case TILES_OK:
    case TILES_ABANDONED:
      e->u_valid = e->linv_valid = false;  // its own eval_tiles, 2089 -> 1377
      if (g == TILES_ABANDONED) return false;  // 2115
      e->have_alpha = true;
      e->u_valid = true;
      return true;
    case TREE_OK:
    case TREE_FAILS_MIDWAY:
      e->u_valid = e->linv_valid = false;  // 2121
      e->factor_consumed = true;           // 2142
      if (g == TREE_FAILS_MIDWAY) return false;
      e->factor_consumed = false;  // 2170
      e->have_alpha = true;        // 2171
      return true;
  }
  return false;
}
// gmb_evaluate with a gradient (2810-2858); `finish_ok`: what factorize_finish finds; `retry`: the launch was abandoned and
// factorize_retry_after_abort (2793-2802) factors again, successfully, the gradient following by tile tasks
void evaluate_grad(Old* e, bool fused, Grad g, bool finish_ok, bool retry) {
  if (!e->r.spec || !e->r.data) return;  // gmb_set_theta refuses
  set_theta(e);
  factorize_enqueue(e, true, fused);
  e->factored = true;  // 2834
  const bool light = fused;
  const bool grad_ok = grad_accumulate(e, g);
  if (!grad_ok && light) {
    e->factored = false;  // 2840
    return;
  }
  if (!factorize_finish(e, finish_ok)) {
    e->have_alpha = false;  // 2848-2850
    e->u_valid = e->linv_valid = false;
    e->factor_consumed = false;
    if (!retry) return;
    factorize_enqueue(e, true, false);
    factorize_finish(e, true);
    grad_accumulate(e, TILES_OK);
  }
}
// refactor_tail (2914-3001)
void refactor_tail(Old* e, bool ok) {
  e->factored = false;
  e->factor_kind = Old::FK_SINGLE;
  e->factor_consumed = false;
  factorize_finish(e, ok);
}
enum Resize { R_OK, R_BUFFER_TOO_SMALL, R_BAIL, R_TAIL_FAILS };
// gmb_append / gmb_truncate -> resize_n (3006-3092)
void resize(Old* e, Resize how) {
  if (!resize_ready(e)) return;
  const bool live = has_live_factor(e);
  e->factored = false;  // 3028-3032
  e->have_alpha = false;
  e->bs_valid = false;
  e->u_valid = e->linv_valid = false;
  if (!live) e->factor_kind = Old::FK_NONE;
  if (how == R_BAIL) {  // 3033-3038
    e->factored = false;
    e->factor_kind = Old::FK_NONE;
    e->r.theta = false;
    return;
  }
  if (!live) {
    if (how == R_BUFFER_TOO_SMALL) e->r.dA = false;  // 3078
    return;
  }
  refactor_tail(e, how != R_TAIL_FAILS);
}
// gmb_dist_set_mode (4476-4497)
void dist_set_mode(Old* e, int mode) {
  const int old = e->r.dist_mode;
  if (old != mode) {
    e->factored = false;
    e->bs_valid = false;
    e->factor_kind = Old::FK_NONE;
  }
  e->r.dist_mode = mode;
  if (mode == 1) {
    if (e->r.dA) {
      e->r.dA = false;
      e->factored = false;
      e->bs_valid = false;
      e->factor_kind = Old::FK_NONE;
    }
  }
}
// gmb_dist_factorize (4505-4509) -> dist_factorize (dist_driver.hpp:336-545) or cap_factorize (dist_capacity.hpp:100-326), the
// communicator sound and the set-up agreed
void dist_factorize(Old* e, bool ok) {
  if (!require_ready(e, false)) return;
  if (e->r.dist_mode == 1) {
    e->r.dAown = true;    // cap_ensure, dist_capacity.hpp:114
    e->factored = false;  // dist_capacity.hpp:125-129
    e->factor_kind = Old::FK_CAPACITY;
    e->factor_consumed = false;
    e->have_alpha = false;
    e->bs_valid = false;
    if (ok) e->factored = true;  // dist_capacity.hpp:324
  } else {
    e->r.dA = true;       // ensure_factor_buffer, dist_driver.hpp:345
    e->factored = false;  // dist_driver.hpp:359-363
    e->factor_kind = Old::FK_REPLICATED;
    e->factor_consumed = false;
    e->have_alpha = false;
    e->bs_valid = false;
    if (ok) e->factored = true;  // dist_driver.hpp:543
  }
}
// gmb_dist_nlml (4511-4514) with a gradient -> dist_nlml (dist_driver.hpp:550-692) or cap_nlml (dist_capacity.hpp:327-539)
void dist_nlml_grad(Old* e, bool ok) {
  if (!require_ready(e, true)) return;
  if (e->r.dist_mode == 1) {
    if (!require_capacity_factor(e)) return;
    if (ok) e->have_alpha = true;  // dist_capacity.hpp:534
  } else {
    if (!require_full_factor(e)) return;
    if (e->factor_consumed) return;  // dist_driver.hpp:564
    e->factor_consumed = true;       // dist_driver.hpp:589
    if (ok) e->have_alpha = true;    // dist_driver.hpp:687
  }
}

void event(Old* e, Event ev) {
  switch (ev) {
    case SET_DATA:
    case SET_DATA_LARGER:  // gmb_set_data (2496-2539)
      e->factored = false;
      e->bs_valid = false;
      e->factor_kind = Old::FK_NONE;
      e->r.theta = false;
      e->u_valid = e->linv_valid = false;        // 2515
      if (ev == SET_DATA_LARGER) e->r.dA = false;  // 2528
      e->r.data = true;
      break;
    case SET_Y:  // gmb_set_y (2541-2553)
      if (!e->r.data) break;
      e->factored = false;
      e->bs_valid = false;
      e->factor_kind = Old::FK_NONE;
      break;
    case SET_KERNEL:  // gmb_set_kernel (2555-2569)
      e->r.spec = true;
      e->r.theta = false;
      e->factored = false;
      e->bs_valid = false;
      e->factor_kind = Old::FK_NONE;
      break;
    case SET_PERIODIC:  // gmb_set_periodic (2571-2597)
      if (!e->r.spec) break;
      e->r.theta = false;
      e->factored = false;
      e->bs_valid = false;
      e->factor_kind = Old::FK_NONE;
      e->u_valid = e->linv_valid = false;
      break;
    case SET_THETA:
      if (!e->r.spec || !e->r.data) break;
      set_theta(e);
      break;
    case FACTORIZE_OK:  // gmb_factorize (2804-2808)
    case FACTORIZE_NOTPD:
    case FACTORIZE_ABANDONED_RETRY_OK:
    case FACTORIZE_ABANDONED_RETRY_FAILS:
    case FACTORIZE_NO_BUFFER:
      if (!require_ready(e, false)) break;
      if (!factorize_enqueue(e, ev != FACTORIZE_NO_BUFFER, false)) break;
      if (factorize_finish(e, ev == FACTORIZE_OK)) break;
      if (ev == FACTORIZE_NOTPD) break;
      factorize_enqueue(e, true, false);  // factorize_retry_after_abort (2793-2802)
      factorize_finish(e, ev == FACTORIZE_ABANDONED_RETRY_OK);
      break;
    case EVALUATE_OK:  // gmb_evaluate without a gradient (2810-2858)
    case EVALUATE_NOTPD:
      if (!e->r.spec || !e->r.data) break;
      set_theta(e);
      factorize_enqueue(e, true, false);
      if (!factorize_finish(e, ev == EVALUATE_OK)) {
        e->have_alpha = false;
        e->u_valid = e->linv_valid = false;
        e->factor_consumed = false;
      }
      break;
    case EVALUATE_GRAD_FUSED_OK: evaluate_grad(e, true, TILES_FUSED_OK, true, false); break;
    case EVALUATE_GRAD_FUSED_FINISH_FAILS: evaluate_grad(e, true, TILES_FUSED_OK, false, false); break;
    case EVALUATE_GRAD_FUSED_GRADIENT_FAILS: evaluate_grad(e, true, TILES_FUSED_FAILS, true, false); break;
    case EVALUATE_GRAD_FUSED_ABANDONED_RETRY_OK: evaluate_grad(e, true, TILES_FUSED_OK, false, true); break;
    case EVALUATE_GRAD_TILES_OK: evaluate_grad(e, false, TILES_OK, true, false); break;
    case EVALUATE_GRAD_TREE_OK: evaluate_grad(e, false, TREE_OK, true, false); break;
    case EVALUATE_GRAD_TREE_FAILS_MIDWAY: evaluate_grad(e, false, TREE_FAILS_MIDWAY, true, false); break;
    case EVALUATE_GRAD_TREE_FAILS_MIDWAY_NOTPD: evaluate_grad(e, false, TREE_FAILS_MIDWAY, false, false); break;
    case NLML_GRAD_TILES_OK:  // gmb_nlml with a gradient (3839-3851)
    case NLML_GRAD_TILES_ABANDONED:
    case NLML_GRAD_TREE_OK:
    case NLML_GRAD_TREE_FAILS_MIDWAY:
      if (!require_ready(e, true) || !require_full_factor(e)) break;
      grad_accumulate(e, ev == NLML_GRAD_TILES_OK ? TILES_OK : ev == NLML_GRAD_TILES_ABANDONED ? TILES_ABANDONED
                         : ev == NLML_GRAD_TREE_OK ? TREE_OK : TREE_FAILS_MIDWAY);
      break;
    case PREDICT:  // predict_sel (3684-...) -> predict_solve_v (3164-3220)
    case PREDICT_JOINT:  // predict_joint_sel / draw_joint_sel -> joint_covariance -> predict_solve_v
      if (!(ev == PREDICT ? predict_ready(e) : joint_ready(e))) break;
      if (predict_takes_gemm_form(e) && !e->linv_valid) e->linv_valid = true;  // 3184-3194
      break;
    case PREDICT_GRAD:  // predict_grad_sel -> resident_alpha (3484-3489) -> backsub_alpha (3447-3464)
      if (!joint_ready(e)) break;
      if (!e->have_alpha && !e->bs_valid) e->bs_valid = true;
      break;
    case RESIZE_OK: resize(e, R_OK); break;
    case RESIZE_OK_BUFFER_TOO_SMALL: resize(e, R_BUFFER_TOO_SMALL); break;
    case RESIZE_BAIL: resize(e, R_BAIL); break;
    case RESIZE_TAIL_FAILS: resize(e, R_TAIL_FAILS); break;
    case DIST_SET_MODE_0: dist_set_mode(e, 0); break;
    case DIST_SET_MODE_1: dist_set_mode(e, 1); break;
    case DIST_FACTORIZE_OK: dist_factorize(e, true); break;
    case DIST_FACTORIZE_FAILS: dist_factorize(e, false); break;
    case DIST_NLML_GRAD_OK: dist_nlml_grad(e, true); break;
    case DIST_NLML_GRAD_FAILS: dist_nlml_grad(e, false); break;
    case DEBUG_ASSUME_FACTORED:  // gmb_debug_assume_factored (4215-4228), the door's environment variable set
      if (!door_opens(e)) break;
      e->factored = true;
      e->factor_consumed = false;
      break;
    case N_EVENTS: break;
  }
}

}  // namespace old_engine

// =====================================================================================================================================
// TODAY: the same entry points in transitions and predicates of FactorState, transcribed from the functions named.
// =====================================================================================================================================
struct New {
  FactorState fs;
  Rest r;
};

namespace new_engine {

bool require_ready(const New* e, bool need_factor) {  // require_ready
  if (!e->r.data || !e->r.spec || !e->r.theta) return false;
  return !(need_factor && !e->fs.valid());
}
bool require_full_factor(const New* e) { return !(e->fs.capacity() || !e->r.dA); }         // require_full_factor
bool require_capacity_factor(const New* e) { return !(!e->fs.capacity() || !e->r.dAown); }  // require_capacity_factor
bool factor_valid(const New* e) { return e->r.data && e->r.theta && e->fs.usable(); }        // gmb_factor_valid
bool has_live_factor(const New* e) { return e->fs.live_single() && e->r.dA; }                // has_live_factor
bool resize_ready(const New* e) {                                                             // resize_ready
  if (!require_ready(e, false)) return false;
  if (e->r.dist_mode != 0 || e->fs.distributed()) return false;
  return !e->fs.valid_but_consumed();
}
bool predict_takes_gemm_form(const New* e) { return e->fs.gemm_form_ready(); }  // predict_takes_gemm_form
bool joint_ready(const New* e) {                                                // joint_ready
  if (!require_ready(e, true)) return false;
  if (e->r.dist_mode != 0 || !e->fs.single()) return false;
  if (!require_full_factor(e)) return false;
  return !e->fs.consumed();
}
bool predict_ready(const New* e) { return require_ready(e, true) && require_full_factor(e) && !e->fs.consumed(); }  // predict_sel
bool copy_factor_refuses(const New* e) { return e->fs.valid() && !require_full_factor(e); }     // gmb_copy_factor
bool copy_alpha_ready(const New* e) { return require_ready(e, false) && e->fs.gradient_alpha(); }  // gmb_copy_alpha
bool door_opens(const New* e) { return !(e->fs.none() || !e->r.theta); }                        // gmb_debug_assume_factored

void set_theta(New* e) {  // gmb_set_theta
  e->fs.inputs_changed();
  e->r.theta = true;
}
bool factorize_enqueue(New* e, bool buffer, bool fused) {  // factorize_enqueue: begin_factorisation, ensure_factor_buffer, eval_tiles
  e->fs.begin(FactorState::SINGLE);
  if (!buffer) return false;
  e->r.dA = true;
  if (fused) e->fs.inverse_rewrites_u();
  return true;
}
bool factorize_finish(New* e, bool ok) {  // factorize_finish: not_accepted at its head, accept_factor at its end
  e->fs.not_accepted();
  if (!ok) return false;
  e->fs.accepted();
  return true;
}
using old_engine::Grad;
bool grad_accumulate(New* e, Grad g) {  // grad_accumulate
  if (e->fs.consumed()) return false;
  switch (g) {
    case old_engine::TILES_FUSED_FAILS: return false;
    case old_engine::TILES_FUSED_OK: e->fs.gradient_left_u_and_alpha(); return true;
    case old_engine::TILES_OK:
    case old_engine::TILES_ABANDONED:
      e->fs.inverse_rewrites_u();  // eval_tiles
      if (g == old_engine::TILES_ABANDONED) return false;
      e->fs.gradient_left_u_and_alpha();
      return true;
    case old_engine::TREE_OK:
    case old_engine::TREE_FAILS_MIDWAY:
      e->fs.inverse_rewrites_u();
      e->fs.consume();
      if (g == old_engine::TREE_FAILS_MIDWAY) return false;
      e->fs.restore();
      return true;
  }
  return false;
}
void evaluate_grad(New* e, bool fused, Grad g, bool finish_ok, bool retry) {  // gmb_evaluate
  if (!e->r.spec || !e->r.data) return;
  set_theta(e);
  factorize_enqueue(e, true, fused);
  e->fs.accepted();
  const bool light = fused;
  const bool grad_ok = grad_accumulate(e, g);
  if (!grad_ok && light) {
    e->fs.not_accepted();
    return;
  }
  if (!factorize_finish(e, finish_ok)) {
    e->fs.gradient_ran_on_garbage();
    if (!retry) return;
    factorize_enqueue(e, true, false);  // factorize_retry_after_abort
    factorize_finish(e, true);
    grad_accumulate(e, old_engine::TILES_OK);
  }
}
using old_engine::Resize;
void resize(New* e, Resize how) {  // gmb_append / gmb_truncate -> resize_n -> refactor_tail
  if (!resize_ready(e)) return;
  const bool live = has_live_factor(e);
  e->fs.resized(live);
  if (how == old_engine::R_BAIL) {
    e->fs.resize_failed();
    e->r.theta = false;
    return;
  }
  if (!live) {
    if (how == old_engine::R_BUFFER_TOO_SMALL) e->r.dA = false;
    return;
  }
  e->fs.begin_tail();  // refactor_tail: begin_factorisation(.., tail)
  factorize_finish(e, how != old_engine::R_TAIL_FAILS);
}
void dist_set_mode(New* e, int mode) {  // gmb_dist_set_mode
  if (e->r.dist_mode != mode) e->fs.inputs_changed();
  e->r.dist_mode = mode;
  if (mode == 1 && e->r.dA) {
    e->r.dA = false;
    e->fs.inputs_changed();
  }
}
void dist_factorize(New* e, bool ok) {  // gmb_dist_factorize -> dist_factorize / cap_factorize: begin_factorisation ... accept_factor
  if (!require_ready(e, false)) return;
  if (e->r.dist_mode == 1) {
    e->r.dAown = true;
    e->fs.begin(FactorState::CAPACITY);
  } else {
    e->r.dA = true;
    e->fs.begin(FactorState::REPLICATED);
  }
  if (ok) e->fs.accepted();
}
void dist_nlml_grad(New* e, bool ok) {  // gmb_dist_nlml -> dist_nlml / cap_nlml
  if (!require_ready(e, true)) return;
  if (e->r.dist_mode == 1) {
    if (!require_capacity_factor(e)) return;
    if (ok) e->fs.alpha_gathered();
  } else {
    if (!require_full_factor(e) || e->fs.consumed()) return;
    e->fs.consume();
    if (ok) e->fs.alpha_gathered();
  }
}

void event(New* e, Event ev) {
  switch (ev) {
    case SET_DATA:
    case SET_DATA_LARGER:  // gmb_set_data
      e->fs.feature_map_changed();
      e->r.theta = false;
      if (ev == SET_DATA_LARGER) e->r.dA = false;
      e->r.data = true;
      break;
    case SET_Y:  // gmb_set_y
      if (e->r.data) e->fs.inputs_changed();
      break;
    case SET_KERNEL:  // gmb_set_kernel
      e->r.spec = true;
      e->r.theta = false;
      e->fs.inputs_changed();
      break;
    case SET_PERIODIC:  // gmb_set_periodic
      if (!e->r.spec) break;
      e->r.theta = false;
      e->fs.feature_map_changed();
      break;
    case SET_THETA:
      if (e->r.spec && e->r.data) set_theta(e);
      break;
    case FACTORIZE_OK:  // gmb_factorize
    case FACTORIZE_NOTPD:
    case FACTORIZE_ABANDONED_RETRY_OK:
    case FACTORIZE_ABANDONED_RETRY_FAILS:
    case FACTORIZE_NO_BUFFER:
      if (!require_ready(e, false)) break;
      if (!factorize_enqueue(e, ev != FACTORIZE_NO_BUFFER, false)) break;
      if (factorize_finish(e, ev == FACTORIZE_OK)) break;
      if (ev == FACTORIZE_NOTPD) break;
      factorize_enqueue(e, true, false);  // factorize_retry_after_abort
      factorize_finish(e, ev == FACTORIZE_ABANDONED_RETRY_OK);
      break;
    case EVALUATE_OK:  // gmb_evaluate without a gradient
    case EVALUATE_NOTPD:
      if (!e->r.spec || !e->r.data) break;
      set_theta(e);
      factorize_enqueue(e, true, false);
      if (!factorize_finish(e, ev == EVALUATE_OK)) e->fs.gradient_ran_on_garbage();
      break;
    case EVALUATE_GRAD_FUSED_OK: evaluate_grad(e, true, old_engine::TILES_FUSED_OK, true, false); break;
    case EVALUATE_GRAD_FUSED_FINISH_FAILS: evaluate_grad(e, true, old_engine::TILES_FUSED_OK, false, false); break;
    case EVALUATE_GRAD_FUSED_GRADIENT_FAILS: evaluate_grad(e, true, old_engine::TILES_FUSED_FAILS, true, false); break;
    case EVALUATE_GRAD_FUSED_ABANDONED_RETRY_OK: evaluate_grad(e, true, old_engine::TILES_FUSED_OK, false, true); break;
    case EVALUATE_GRAD_TILES_OK: evaluate_grad(e, false, old_engine::TILES_OK, true, false); break;
    case EVALUATE_GRAD_TREE_OK: evaluate_grad(e, false, old_engine::TREE_OK, true, false); break;
    case EVALUATE_GRAD_TREE_FAILS_MIDWAY: evaluate_grad(e, false, old_engine::TREE_FAILS_MIDWAY, true, false); break;
    case EVALUATE_GRAD_TREE_FAILS_MIDWAY_NOTPD: evaluate_grad(e, false, old_engine::TREE_FAILS_MIDWAY, false, false); break;
    case NLML_GRAD_TILES_OK:  // gmb_nlml with a gradient
    case NLML_GRAD_TILES_ABANDONED:
    case NLML_GRAD_TREE_OK:
    case NLML_GRAD_TREE_FAILS_MIDWAY:
      if (!require_ready(e, true) || !require_full_factor(e)) break;
      grad_accumulate(e, ev == NLML_GRAD_TILES_OK ? old_engine::TILES_OK : ev == NLML_GRAD_TILES_ABANDONED ? old_engine::TILES_ABANDONED
                         : ev == NLML_GRAD_TREE_OK ? old_engine::TREE_OK : old_engine::TREE_FAILS_MIDWAY);
      break;
    case PREDICT:        // predict_sel -> predict_solve_v
    case PREDICT_JOINT:  // predict_joint_sel / draw_joint_sel -> joint_covariance -> predict_solve_v
      if (!(ev == PREDICT ? predict_ready(e) : joint_ready(e))) break;
      if (predict_takes_gemm_form(e) && e->fs.linv_missing()) e->fs.linv_transposed();
      break;
    case PREDICT_GRAD:  // predict_grad_sel -> resident_alpha -> backsub_alpha
      if (!joint_ready(e)) break;
      if (e->fs.needs_backsub()) e->fs.back_substituted();
      break;
    case RESIZE_OK: resize(e, old_engine::R_OK); break;
    case RESIZE_OK_BUFFER_TOO_SMALL: resize(e, old_engine::R_BUFFER_TOO_SMALL); break;
    case RESIZE_BAIL: resize(e, old_engine::R_BAIL); break;
    case RESIZE_TAIL_FAILS: resize(e, old_engine::R_TAIL_FAILS); break;
    case DIST_SET_MODE_0: dist_set_mode(e, 0); break;
    case DIST_SET_MODE_1: dist_set_mode(e, 1); break;
    case DIST_FACTORIZE_OK: dist_factorize(e, true); break;
    case DIST_FACTORIZE_FAILS: dist_factorize(e, false); break;
    case DIST_NLML_GRAD_OK: dist_nlml_grad(e, true); break;
    case DIST_NLML_GRAD_FAILS: dist_nlml_grad(e, false); break;
    case DEBUG_ASSUME_FACTORED:  // gmb_debug_assume_factored
      if (door_opens(e)) e->fs.assume_factored();
      break;
    case N_EVENTS: break;
  }
}

}  // namespace new_engine

// =====================================================================================================================================
// the comparison and the replay
// =====================================================================================================================================

// the name of the first thing that differs, or nullptr
static const char* difference(const Old& o, const New& n) {
  const FactorState& f = n.fs;
  // the seven values
  if (o.factored != f.valid()) return "factored";
  if (o.factor_kind != (int)f.kind()) return "factor_kind";
  if (o.factor_consumed != f.consumed()) return "factor_consumed";
  if (o.have_alpha != f.gradient_alpha()) return "have_alpha";
  if (o.bs_valid != f.backsub_alpha()) return "bs_valid";
  if (o.u_valid != f.u_resident()) return "u_valid";
  if (o.linv_valid != !f.linv_missing()) return "linv_valid";
  if (!(o.r == n.r)) return "the rest of the engine";
  // every predicate against the expression it replaced
  if ((o.factored && !o.factor_consumed) != f.usable()) return "usable";
  if ((o.factored && o.factor_consumed) != f.valid_but_consumed()) return "valid_but_consumed";
  if ((o.factored && o.factor_kind == Old::FK_SINGLE && !o.factor_consumed) != f.live_single()) return "live_single";
  if ((o.factor_kind == Old::FK_NONE) != f.none()) return "none";
  if ((o.factor_kind == Old::FK_SINGLE) != f.single()) return "single";
  if ((o.factor_kind == Old::FK_CAPACITY) != f.capacity()) return "capacity";
  if ((o.factor_kind == Old::FK_REPLICATED || o.factor_kind == Old::FK_CAPACITY) != f.distributed()) return "distributed";
  if ((o.u_valid && o.have_alpha && o.factor_kind == Old::FK_SINGLE) != f.gemm_form_ready()) return "gemm_form_ready";
  if ((!o.have_alpha && !o.bs_valid) != f.needs_backsub()) return "needs_backsub";
  // ... and the callers' compound forms
  if (old_engine::require_ready(&o, true) != new_engine::require_ready(&n, true)) return "require_ready";
  if (old_engine::require_full_factor(&o) != new_engine::require_full_factor(&n)) return "require_full_factor";
  if (old_engine::require_capacity_factor(&o) != new_engine::require_capacity_factor(&n)) return "require_capacity_factor";
  if (old_engine::factor_valid(&o) != new_engine::factor_valid(&n)) return "gmb_factor_valid";
  if (old_engine::has_live_factor(&o) != new_engine::has_live_factor(&n)) return "has_live_factor";
  if (old_engine::resize_ready(&o) != new_engine::resize_ready(&n)) return "resize_ready";
  if (old_engine::predict_takes_gemm_form(&o) != new_engine::predict_takes_gemm_form(&n)) return "predict_takes_gemm_form";
  if (old_engine::joint_ready(&o) != new_engine::joint_ready(&n)) return "joint_ready";
  if (old_engine::predict_ready(&o) != new_engine::predict_ready(&n)) return "predict_sel's guards";
  if (old_engine::copy_factor_refuses(&o) != new_engine::copy_factor_refuses(&n)) return "gmb_copy_factor's guard";
  if (old_engine::copy_alpha_ready(&o) != new_engine::copy_alpha_ready(&n)) return "gmb_copy_alpha's guard";
  if (old_engine::door_opens(&o) != new_engine::door_opens(&n)) return "gmb_debug_assume_factored's guard";
  return nullptr;
}

// the oracle's state as a number (both states are equal whenever this is asked)
static unsigned pack(const Old& o) {
  unsigned k = (unsigned)o.factor_kind;  // 2 bits
  const bool bits[] = {o.factored, o.factor_consumed, o.have_alpha, o.bs_valid, o.u_valid, o.linv_valid,
                       o.r.data, o.r.spec, o.r.theta, o.r.dist_mode != 0, o.r.dA, o.r.dAown};
  for (bool b : bits) k = (k << 1) | (b ? 1u : 0u);
  return k;  // < 2^14
}

static std::vector<signed char> expanded(1u << 14, -1);  // the most events-to-go a state has been expanded with
static std::vector<Event> path;
static long long applied = 0;

static void replay(const Old& o, const New& n, int to_go) {
  if (to_go == 0) return;
  const unsigned key = pack(o);
  if (expanded[key] >= to_go) return;
  expanded[key] = (signed char)to_go;
  for (int ev = 0; ev < N_EVENTS; ++ev) {
    Old o2 = o;
    New n2 = n;
    old_engine::event(&o2, (Event)ev);
    new_engine::event(&n2, (Event)ev);
    ++applied;
    path.push_back((Event)ev);
    if (const char* what = difference(o2, n2)) {
      printf("DIFFERENCE in %s after:", what);
      for (Event p : path) printf(" %s", EVENT_NAMES[p]);
      printf("\n");
      exit(1);
    }
    replay(o2, n2, to_go - 1);
    path.pop_back();
  }
}

int main() {
  Old o;
  New n;
  if (const char* what = difference(o, n)) {
    printf("DIFFERENCE in %s on a freshly created engine\n", what);
    return 1;
  }
  replay(o, n, MAX_EVENTS);
  int states = 0, marks = 0;
  std::vector<bool> seen_marks(1u << 8, false);
  for (unsigned k = 0; k < expanded.size(); ++k)
    if (expanded[k] >= 0) {
      ++states;
      seen_marks[k >> 6] = true;
    }
  for (bool b : seen_marks) marks += b ? 1 : 0;
  printf("factor_state_check: every sequence of up to %d of %d events agrees: %d engine states (%d values of the seven marks), "
         "%lld events replayed\n", MAX_EVENTS, (int)N_EVENTS, states, marks, applied);
  return 0;
}
