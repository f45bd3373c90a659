// term_walk_check.cpp -- the walk over an additive model's covariance terms (gumbi_amd/csrc/term_walk.hpp: the very header engine.hip
// walks its terms with) driven with recording stubs, as a stand-alone program for the sanitizers.  No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/term_walk_check.cpp -o /tmp/term_walk_check
//   /tmp/term_walk_check
//
// Every case names the term at which a body or a preparation fails (and with what), runs the walk and compares the exact sequence
// of calls and the returned status:
//   * one term: the body alone, no preparation at all;
//   * three terms: body0, prep1, body1, prep2, body2, prep0;
//   * a failing body (term 0: nothing was re-prepared, nothing is put back; term 1: prep0 follows, the body's status returns);
//   * a failing preparation: the restore is still attempted, the first status returns;
//   * a failing restore: reported after a clean walk, never in place of an earlier error.
// One line per case; exit status 0 when all agree (tests/test_term_walk_cpu.py builds and runs it without the sanitizers).
#include <cstdio>
#include <string>

#include "../gumbi_amd/csrc/term_walk.hpp"

static int failures = 0;

struct Case {
  const char* name;
  int nterms;
  int body_fails_at, body_rc;  // -1: no body fails
  int prep_fails_at, prep_rc;  // -1: no preparation fails; 0: the restore
  const char* calls;           // expected
  int rc;                      // expected
};

static void run(const Case& c) {
  std::string log;
  auto note = [&](const char* what, int t) {
    if (!log.empty()) log += ' ';
    log += what + std::to_string(t);
  };
  const int rc = gmb::for_each_term(
      c.nterms,
      [&](int t) {
        note("prep", t);
        return t == c.prep_fails_at ? c.prep_rc : 0;
      },
      [&](int t) {
        note("body", t);
        return t == c.body_fails_at ? c.body_rc : 0;
      });
  const bool ok = log == c.calls && rc == c.rc;
  std::printf("%s %-48s rc %3d  [%s]\n", ok ? "ok  " : "FAIL", c.name, rc, log.c_str());
  if (!ok) {
    std::printf("     expected                                         rc %3d  [%s]\n", c.rc, c.calls);
    ++failures;
  }
}

int main() {
  const Case cases[] = {
      {"no terms", 0, -1, 0, -1, 0, "", 0},
      {"one term", 1, -1, 0, -1, 0, "body0", 0},
      {"one term, body fails", 1, 0, -3, -1, 0, "body0", -3},
      {"two terms", 2, -1, 0, -1, 0, "body0 prep1 body1 prep0", 0},
      {"three terms", 3, -1, 0, -1, 0, "body0 prep1 body1 prep2 body2 prep0", 0},
      {"three terms, body 0 fails (nothing to restore)", 3, 0, -3, -1, 0, "body0", -3},
      {"three terms, body 1 fails", 3, 1, -3, -1, 0, "body0 prep1 body1 prep0", -3},
      {"three terms, body 2 fails", 3, 2, -3, -1, 0, "body0 prep1 body1 prep2 body2 prep0", -3},
      {"three terms, preparation 1 fails", 3, -1, 0, 1, -5, "body0 prep1 prep0", -5},
      {"three terms, preparation 2 fails", 3, -1, 0, 2, -5, "body0 prep1 body1 prep2 prep0", -5},
      {"three terms, the restore fails", 3, -1, 0, 0, -7, "body0 prep1 body1 prep2 body2 prep0", -7},
      {"three terms, body 1 and the restore fail", 3, 1, -3, 0, -7, "body0 prep1 body1 prep0", -3},
  };
  for (const Case& c : cases) run(c);
  std::printf("%s\n", failures ? "FAILED" : "all cases agree");
  return failures ? 1 : 0;
}
