// term_select_check.cpp -- the walk over a SELECTION of an additive model's covariance terms (gumbi_amd/csrc/term_walk.hpp: the very
// header engine.hip walks its terms with) driven with recording stubs, as a stand-alone program for the sanitizers.  No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/term_select_check.cpp -o /tmp/term_select_check
//   /tmp/term_select_check
//
// For T = 1, 3, 5 terms and EVERY mask of T bits (the empty one included), without a failure and with a body or a preparation --
// the restore among them -- failing at every place it can, the record of the calls is checked against the rules of the walk:
//   * the bodies that ran are the selected terms in ascending order (all of them, or up to the failure);
//   * prep t comes directly before body t for every selected t > 0, and nowhere else;
//   * prep 0 -- the restore -- is the last call if and only if a later term was prepared, whether or not something failed;
//   * a selection of term 0 alone, and the empty one, prepare nothing;
//   * the first error is what the walk returns; the restore's own only after a clean walk;
//   * the mask with all T bits set, and masks with further bits beyond T, leave the record of the walk without a mask.
// One line per T; exit status 0 when all agree (tests/test_term_select_cpu.py builds and runs it without the sanitizers).
#include <cstdio>
#include <string>
#include <vector>

#include "../gumbi_amd/csrc/term_walk.hpp"

static int failures = 0;
static long checked = 0;

struct Call {
  char what;  // 'p' or 'b'
  int t;
};

struct Fault {
  int body_at = -1, body_rc = 0;  // -1: no body fails
  int prep_at = -1, prep_rc = 0;  // -1: no preparation fails; 0: the restore
};

static std::string show(const std::vector<Call>& log) {
  std::string s;
  for (const Call& c : log) s += std::string(s.empty() ? "" : " ") + (c.what == 'p' ? "prep" : "body") + std::to_string(c.t);
  return s;
}

template <typename Walk>
static int record(Walk&& walk, const Fault& f, std::vector<Call>& log) {
  log.clear();
  return walk(
      [&](int t) {
        log.push_back({'p', t});
        return t == f.prep_at ? f.prep_rc : 0;
      },
      [&](int t) {
        log.push_back({'b', t});
        return t == f.body_at ? f.body_rc : 0;
      });
}

static void complain(int T, unsigned mask, const Fault& f, const std::vector<Call>& log, int rc, const char* why) {
  std::printf("FAIL T %d mask 0x%x body@%d prep@%d: %s -- rc %d [%s]\n", T, mask, f.body_at, f.prep_at, why, rc, show(log).c_str());
  ++failures;
}

// the rules, read off the record
static void check(int T, unsigned mask, const Fault& f) {
  std::vector<Call> log;
  const int rc = record([&](auto&& p, auto&& b) { return gmb::for_each_term(T, mask, p, b); }, f, log);
  ++checked;
  std::vector<int> selected;
  for (int t = 0; t < T; ++t)
    if ((mask >> t) & 1u) selected.push_back(t);

  // walk the record: an optional "prep t" before every body t > 0, bodies ascending through the selection, a trailing "prep 0"
  size_t i = 0, k = 0;
  int first_error = 0;
  bool moved = false;
  while (k < selected.size() && !first_error) {
    const int t = selected[k];
    if (t > 0) {
      if (i >= log.size() || log[i].what != 'p' || log[i].t != t) return complain(T, mask, f, log, rc, "a selected term > 0 was not prepared first");
      ++i;
      moved = true;
      if (t == f.prep_at && f.prep_rc) {
        first_error = f.prep_rc;
        break;
      }
    }
    if (i >= log.size() || log[i].what != 'b' || log[i].t != t) return complain(T, mask, f, log, rc, "the bodies are not the selected terms in ascending order");
    ++i;
    if (t == f.body_at && f.body_rc) first_error = f.body_rc;
    ++k;
  }
  if (moved) {
    if (i + 1 != log.size() || log[i].what != 'p' || log[i].t != 0) return complain(T, mask, f, log, rc, "term 0's preparation does not follow as the last call");
    if (!first_error && f.prep_at == 0) first_error = f.prep_rc;
  } else if (i != log.size()) {
    return complain(T, mask, f, log, rc, "calls beyond the selection (nothing was prepared: nothing is to be put back)");
  }
  if (rc != first_error) return complain(T, mask, f, log, rc, "the first error is not what the walk returned");
  if ((mask & ((1u << T) - 1u)) == 1u || selected.empty())
    for (const Call& c : log)
      if (c.what == 'p') return complain(T, mask, f, log, rc, "a selection without a later term prepared something");
}

// all bits (and bits beyond T): the record of the walk without a mask
static void check_all_bits(int T, const Fault& f) {
  std::vector<Call> plain, masked;
  const int rc0 = record([&](auto&& p, auto&& b) { return gmb::for_each_term(T, p, b); }, f, plain);
  for (unsigned mask : {(1u << T) - 1u, gmb::ALL_TERMS, ((1u << T) - 1u) | (1u << (T + 2))}) {
    const int rc1 = record([&](auto&& p, auto&& b) { return gmb::for_each_term(T, mask, p, b); }, f, masked);
    ++checked;
    if (rc0 != rc1 || show(plain) != show(masked)) {
      complain(T, mask, f, masked, rc1, "differs from the walk without a mask");
      std::printf("     without a mask: rc %d [%s]\n", rc0, show(plain).c_str());
    }
  }
}

int main() {
  for (int T : {1, 3, 5}) {
    std::vector<Fault> faults(1);  // none
    for (int t = 0; t < T; ++t) {
      Fault fb, fp, fboth;
      fb.body_at = t, fb.body_rc = -3;
      fp.prep_at = t, fp.prep_rc = -5;  // t == 0: the restore
      fboth.body_at = t, fboth.body_rc = -3, fboth.prep_at = 0, fboth.prep_rc = -7;
      faults.push_back(fb);
      faults.push_back(fp);
      faults.push_back(fboth);
      for (int u = 1; u < T; ++u) {  // a body and a later (or earlier) preparation both fail
        Fault f2 = fb;
        f2.prep_at = u, f2.prep_rc = -5;
        faults.push_back(f2);
      }
    }
    const long before = checked;
    for (unsigned mask = 0; mask < (1u << T); ++mask)
      for (const Fault& f : faults) check(T, mask, f);
    for (const Fault& f : faults) check_all_bits(T, f);
    std::printf("T = %d: %u masks x %zu fault placements, %ld walks checked\n", T, 1u << T, faults.size(), checked - before);
  }
  // the first selected term: where a storing pass switches
  for (unsigned mask = 1; mask < 32; ++mask) {
    int want = 0;
    while (!((mask >> want) & 1u)) ++want;
    if (gmb::first_term(mask) != want) {
      std::printf("FAIL first_term(0x%x) = %d, expected %d\n", mask, gmb::first_term(mask), want);
      ++failures;
    }
  }
  std::printf("%s\n", failures ? "FAILED" : "all cases agree");
  return failures ? 1 : 0;
}
