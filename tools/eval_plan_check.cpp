// eval_plan_check.cpp -- gumbi_amd/csrc/eval_plan.hpp (the very header gmb_evaluate plans with) against a frozen copy of the two
// places that used to decide the same things on loose fields of the engine, as a stand-alone program for the sanitizers.
// No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/eval_plan_check.cpp -o /tmp/eval_plan_check
//   /tmp/eval_plan_check
//
// old_plan: the assignments of gmb_set_theta and factorize_enqueue as they stood at commit 4228f16, verbatim and in that order, on
// loose variables named after the engine's fields (THE ORACLE -- frozen, never edited to follow the engine; the line numbers in its
// comments are that commit's).  gmb_evaluate raised eval_call and passed with_grad from the same argument (grad != nullptr).
//
// Every case of the grid below goes through both; light, prezero, inline_prep and events must be equal, and the memset's cover of
// the gradient accumulators (gacc_zeroed, which has no field in the plan) must equal light.  The first difference prints its inputs
// and ends the program with status 1 (tests/test_eval_plan_cpu.py builds and runs it without the sanitizers).
#include <cstdint>
#include <cstdio>

#include "../gumbi_amd/csrc/eval_plan.hpp"

using gmb::EvalPlan;
using gmb::EvalPlanIn;

// =====================================================================================================================================
// THE ORACLE.  Frozen.
// =====================================================================================================================================
struct Old {
  bool light = false, gacc_zeroed = false, prezeroed = false, prep_deferred = false, fe_recorded = false;
};

static Old old_plan(bool grad, bool eval_will_fuse, int ct_lose, int terms_size, int64_t Nr, int64_t Np, int64_t inline_prep_max_rows,
                    bool naive_leaf, bool profiling) {
  Old e;
  // gmb_evaluate (engine.hip:2804, 2810)
  const bool eval_call = grad;
  const bool with_grad = grad;
  // gmb_set_theta (engine.hip:2591-2603)
  e.prezeroed = false;
  if (eval_call && eval_will_fuse && ct_lose == 0) {
    e.prezeroed = true;
  }
  e.prep_deferred = e.prezeroed && terms_size == 1 && Nr <= inline_prep_max_rows && !naive_leaf;
  // factorize_enqueue (engine.hip:2707-2716)
  const bool fused = with_grad && eval_will_fuse;
  e.light = eval_call && fused;
  const bool events = !(e.light && !profiling && Np < 4096);
  e.fe_recorded = events;
  e.prezeroed = e.prezeroed && e.light;
  e.gacc_zeroed = e.light;
  return e;
}

int main() {
  const int64_t NR[3] = {128, 4096, 4224}, NP[3] = {128, 3968, 4096};
  const int64_t inline_prep_max_rows = 4096;  // the engine's
  long cases = 0;
  for (int grad = 0; grad < 2; ++grad)
    for (int fuse = 0; fuse < 2; ++fuse)
      for (int lose = 0; lose < 2; ++lose)
        for (int terms = 1; terms <= 3; ++terms)
          for (int64_t Nr : NR)
            for (int64_t Np : NP)
              for (int naive = 0; naive < 2; ++naive)
                for (int prof = 0; prof < 2; ++prof) {
                  const Old o = old_plan(grad, fuse, lose, terms, Nr, Np, inline_prep_max_rows, naive, prof);
                  EvalPlanIn in;
                  in.with_grad = grad;
                  in.will_fuse = fuse;
                  in.ct_lose = lose;
                  in.nterms = terms;
                  in.Nr = Nr;
                  in.Np = Np;
                  in.inline_prep_max_rows = inline_prep_max_rows;
                  in.naive_leaf = naive;
                  in.profiling = prof;
                  const EvalPlan p = gmb::plan_evaluation(in);
                  ++cases;
                  if (p.light == o.light && p.prezero == o.prezeroed && p.inline_prep == o.prep_deferred && p.events == o.fe_recorded &&
                      o.gacc_zeroed == p.light)
                    continue;
                  printf("DIFFERENCE at grad=%d will_fuse=%d ct_lose=%d terms=%d Nr=%lld Np=%lld naive_leaf=%d profiling=%d\n", grad, fuse, lose,
                         terms, (long long)Nr, (long long)Np, naive, prof);
                  printf("  old: light=%d prezeroed=%d prep_deferred=%d fe_recorded=%d gacc_zeroed=%d\n", o.light, o.prezeroed, o.prep_deferred,
                         o.fe_recorded, o.gacc_zeroed);
                  printf("  new: light=%d prezero=%d inline_prep=%d events=%d\n", p.light, p.prezero, p.inline_prep, p.events);
                  return 1;
                }
  const EvalPlan plain;  // what gmb_factorize, the retry, the bordered update and the multi-GPU drivers run with
  if (plain.light || plain.prezero || plain.inline_prep || !plain.events) {
    printf("DIFFERENCE: the default plan is not the plain one\n");
    return 1;
  }
  printf("eval_plan_check: %ld cases, plan_evaluation equals the two-site logic in all of them\n", cases);
  return 0;
}
