// term_walk.hpp -- the order in which an additive model's covariance terms are visited.
//
// The engine keeps ONE prepared copy of the training points, and between calls it holds term 0's preparation.  A pass over the
// terms re-prepares that copy for every further term; for_each_term is the one place that does so and the one place that puts
// term 0's preparation back -- on the normal end, when a body fails and when a preparation itself fails.
//
// No engine types and no HIP: tools/term_walk_check.cpp drives this very header with recording stubs.
#pragma once

namespace gmb {

constexpr unsigned ALL_TERMS = ~0u;  // the selection that visits every term

// The walk over a SELECTION of the terms: bit t of `mask` selects term t (bits at or beyond nterms are ignored).  body(t) runs for
// the selected t in ascending order, prepare_train(t) before every selected t > 0; both return 0 or an error, and the first error
// ends the walk and is what the walk returns.  Once a prepare_train(t > 0) has been issued, prepare_train(0) follows on EVERY way
// out (its own failure is reported only when nothing failed before it).  A selection of term 0 alone: no prepare_train at all.
template <typename PrepareTrain, typename Body>
int for_each_term(int nterms, unsigned mask, PrepareTrain&& prepare_train, Body&& body) {
  int rc = 0;
  bool moved = false;  // the resident preparation is (or may be) a later term's
  for (int t = 0; t < nterms && t < 32 && !rc; ++t) {
    if (!((mask >> t) & 1u)) continue;
    if (t > 0) {
      moved = true;
      if ((rc = prepare_train(t))) break;
    }
    rc = body(t);
  }
  if (moved) {
    const int back = prepare_train(0);
    if (!rc) rc = back;
  }
  return rc;
}

// every term: body(t) for t = 0 .. nterms - 1.  One term: no prepare_train at all.
template <typename PrepareTrain, typename Body>
int for_each_term(int nterms, PrepareTrain&& prepare_train, Body&& body) {
  return for_each_term(nterms, ALL_TERMS, prepare_train, body);
}

// the lowest selected term of a non-empty selection: the pass that stores where the later ones accumulate
inline int first_term(unsigned mask) {
  int t = 0;
  while (t < 31 && !((mask >> t) & 1u)) ++t;
  return t;
}

}  // namespace gmb
