// factor_state.hpp -- what the engine still holds of its last factorisation, and whether it may be used.
//
// Seven values and an epoch counter, written ONLY by the transitions below and read through the predicates: an entry point names what happened and the
// transition decides which values fall; tests of buffers stay with the callers.  No engine types and no HIP:
// tools/factor_state_check.cpp replays every short sequence of ABI calls through this header and a frozen copy of what it replaced.
#pragma once

namespace gmb {

class FactorState {
 public:
  // the path that produced the factorisation: only the capacity driver's leaves NO complete factor in the factor buffer
  enum Kind { NONE = 0, SINGLE = 1, REPLICATED = 2, CAPACITY = 3 };

  // ---- transitions ----
  // theta, y, the kernel or the distribution mode changed.  (alpha, U and L^-1 keep their marks: every reader of them asks for a
  // valid factorisation or for the SINGLE kind first -- except gmb_copy_alpha, which hands out the previous alpha.)
  void inputs_changed() { valid_ = bs_ = false; kind_ = NONE; ++epoch_; }
  // the data or the periodic feature map changed: the inverse factor belongs to the old prepared coordinates as well
  void feature_map_changed() { inputs_changed(); u_ = linv_ = false; }
  // a whole factorisation starts.  (The multi-GPU kinds leave U and L^-1 marked: the GEMM form asks for the SINGLE kind.)
  void begin(Kind k) {
    valid_ = consumed_ = alpha_ = bs_ = false;
    kind_ = k;
    ++epoch_;
    if (k == SINGLE) u_ = linv_ = false;
  }
  // the tail of the bordered factor starts, behind resized(), which has dropped alpha, U and L^-1 already
  void begin_tail() { valid_ = consumed_ = false; kind_ = SINGLE; ++epoch_; }
  // N changed under the engine; `live`: a live single factor is carried over (its kind stays for begin_tail)
  void resized(bool live) {
    valid_ = alpha_ = bs_ = u_ = linv_ = false;
    if (!live) kind_ = NONE;
    ++epoch_;
  }
  void resize_failed() { valid_ = false; kind_ = NONE; ++epoch_; }
  void accepted() { valid_ = true; }  // the host has looked at the results (gmb_evaluate: will look, and takes it back)
  void not_accepted() { valid_ = false; ++epoch_; }
  void gradient_left_u_and_alpha() { alpha_ = u_ = true; }   // the tile path: alpha = Sigma^-1 y and U = L^-T stay, L is intact
  void inverse_rewrites_u() { u_ = linv_ = false; }          // ... and Sigma^-1 takes the buffer of L^-1
  void consume() { consumed_ = true; }                       // U takes the place of the factor's diagonal blocks ...
  void restore() { consumed_ = false; alpha_ = true; }       // ... and L is back, alpha beside it (launch tree)
  void alpha_gathered() { alpha_ = true; }                   // the multi-GPU gradients: alpha of every rank's rows
  void gradient_ran_on_garbage() { alpha_ = u_ = linv_ = consumed_ = false; }  // behind a factorisation that failed (gmb_evaluate)
  void linv_transposed() { linv_ = true; }                   // the first GEMM-form prediction: L^-1 = U^T
  void back_substituted() { bs_ = true; }                    // alpha = L^-T v, for the states without a gradient's
  void assume_factored() { valid_ = true; consumed_ = false; ++epoch_; }  // the timing tools' debug door

  // ---- predicates ----
  bool valid() const { return valid_; }
  bool consumed() const { return consumed_; }
  bool usable() const { return valid_ && !consumed_; }
  bool valid_but_consumed() const { return valid_ && consumed_; }
  bool live_single() const { return valid_ && kind_ == SINGLE && !consumed_; }  // (+ the caller's look at the factor buffer)
  Kind kind() const { return kind_; }
  bool none() const { return kind_ == NONE; }
  bool single() const { return kind_ == SINGLE; }
  bool capacity() const { return kind_ == CAPACITY; }
  bool distributed() const { return kind_ == REPLICATED || kind_ == CAPACITY; }
  bool gemm_form_ready() const { return u_ && alpha_ && kind_ == SINGLE; }  // (+ the caller's look at the workspaces)
  bool gradient_alpha() const { return alpha_; }          // the resident alpha is a gradient's
  bool needs_backsub() const { return !alpha_ && !bs_; }  // ... and none is resident at all
  bool linv_missing() const { return !linv_; }
  bool backsub_alpha() const { return bs_; }  // (these two: read on their own by the check program only)
  bool u_resident() const { return u_; }
  // Counts the transitions after which (data, theta, factor) may be another: what is derived from a factorisation and kept
  // beside it (the pathwise draws' A, pathwise.hpp) remembers the epoch it was made in and is stale in any other.
  unsigned epoch() const { return epoch_; }

 private:
  Kind kind_ = NONE;
  bool valid_ = false;     // a complete factorisation of the current (data, kernel, theta) has been accepted
  bool consumed_ = false;  // U = L^-T sits in the factor's diagonal blocks
  bool alpha_ = false;     // alpha = Sigma^-1 y of this factorisation, left by a gradient
  bool bs_ = false;        // alpha by back substitution
  bool u_ = false;         // U = L^-T in the factor buffer's upper triangle + its diagonal blocks' own buffer
  bool linv_ = false;      // L^-1 = U^T in the buffer Sigma^-1 had
  unsigned epoch_ = 0;     // see epoch()
};

}  // namespace gmb
