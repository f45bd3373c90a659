// eval_plan.hpp -- how ONE evaluation (gmb_evaluate) or factorisation runs, decided once before its first launch.
//
// The plan is an argument: gmb_evaluate makes it and hands it down to every function that acts on it; nothing of it is kept in
// the engine, so nothing has to be reset when a call ends, however it ends.  No engine types and no HIP:
// tools/eval_plan_check.cpp compares plan_evaluation with a frozen copy of the two places that used to decide the same things.
#pragma once

#include <cstdint>

namespace gmb {

// what the decision reads: the call's own argument, and the engine's sizes and switches as they stand when the call begins
struct EvalPlanIn {
  bool with_grad = false;  // the caller wants the gradient with the value
  bool will_fuse = false;  // eval_will_fuse: at this size and with these schemes the gradient rides in the factorisation's launch
  int ct_lose = 0;         // the fault injection is armed (gmb_debug_chol_lose_tickets)
  int nterms = 1;          // covariance terms of the model
  int64_t Nr = 0, Np = 0;  // padded rows / columns of the factor
  int64_t inline_prep_max_rows = 0;
  bool naive_leaf = false;
  bool profiling = false;
};

// A default-constructed plan is the PLAIN one: gmb_factorize, the retry after an abandoned tile launch, the bordered update and
// the multi-GPU drivers run that way.
struct EvalPlan {
  // the fused evaluation launch, with one memset for scalars + gradient accumulators and everything the host wants landing
  // through eval_land_kernel / grad_finish_kernel at the end of the gradient
  bool light = false;
  // ... and no memset at all: the launch that prepares the points clears the scalar block and the tile launch's control words
  bool prezero = false;
  // ... and that launch is the covariance build itself (CovTileArgs::inline_prep): no prep_points launch
  bool inline_prep = false;
  // the events around the covariance build and the Cholesky are recorded (kbuild_ms, chol_ms)
  bool events = true;
};

// The progress of ONE factorisation, on the stack of the entry point that runs it (gmb_factorize, gmb_evaluate, the bordered
// update) and passed by reference: how it runs and what has happened so far.  The retry after an abandoned launch makes its own.
struct FactorJob {
  EvalPlan plan;
  bool build_reached = false;    // the covariance build was reached (inline_prep: the points are prepared)
  bool fused_pending = false;    // it carries INV / ZZ tasks: Sigma^-1 and the alpha parts come with it; no gradient has taken them yet
  bool in_flight = false;        // enqueued, and the host has not looked at it yet
  bool events_recorded = false;  // the engine's phase events belong to it
};

inline EvalPlan plan_evaluation(const EvalPlanIn& in) {
  const bool light = in.with_grad && in.will_fuse;
  const bool prezero = light && in.ct_lose == 0;
  const bool inline_prep = prezero && in.nterms == 1 && in.Nr <= in.inline_prep_max_rows && !in.naive_leaf;
  // below 4096 rows and without gmb_set_profiling: six event records were ~30 us of a 380 us evaluation at N = 392
  const bool events = !(light && !in.profiling && in.Np < 4096);
  return EvalPlan{light, prezero, inline_prep, events};
}

}  // namespace gmb
