// kernel_dispatch_check.cpp -- the dispatch of (kernel kind, padded width) to template constants (gumbi_amd/csrc/kernel_dispatch.hpp:
// the very header engine.hip launches its covariance kernels through) driven with a recording functor, as a stand-alone program
// for the sanitizers.  No GPU, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/kernel_dispatch_check.cpp -o /tmp/kernel_dispatch_check
//   /tmp/kernel_dispatch_check
//
// For every kind in -1 .. 5 and every nc_pad in 0 .. 17 and 32:
//   * a known kind (0 .. 4): exactly one call, with K = kind and NC = nc_pad where nc_pad is 1, 2, 4 or 8 and 16 otherwise; true returns;
//   * an unknown kind: no call, false returns.
// For every n in 0 .. 16, pick_nc(n) holds n columns and is a width the dispatcher maps to itself.
// One line per kind; exit status 0 when all agree (tests/test_kernel_dispatch_cpu.py builds and runs it without the sanitizers).
#include <cstdio>
#include <utility>
#include <vector>

#include "../gumbi_amd/csrc/kernel_dispatch.hpp"

static int failures = 0;

struct Recorder {
  std::vector<std::pair<int, int>> calls;
  template <typename K, typename NC>
  void operator()(K, NC) {
    calls.emplace_back(K::value, NC::value);
  }
};

static int expected_nc(int nc_pad) { return nc_pad == 1 || nc_pad == 2 || nc_pad == 4 || nc_pad == 8 ? nc_pad : 16; }

int main() {
  std::vector<int> widths;
  for (int nc = 0; nc <= 17; ++nc) widths.push_back(nc);
  widths.push_back(32);
  for (int kind = -1; kind <= 5; ++kind) {
    const bool known = kind >= 0 && kind <= 4;
    int bad = 0;
    for (int nc_pad : widths) {
      Recorder r;
      const bool found = gmb::with_kind_nc(kind, nc_pad, r);
      const bool ok = known ? found && r.calls.size() == 1 && r.calls[0] == std::make_pair(kind, expected_nc(nc_pad))
                            : !found && r.calls.empty();
      if (!ok) {
        std::printf("     kind %d nc_pad %d: returned %d after %zu calls", kind, nc_pad, (int)found, r.calls.size());
        for (const auto& c : r.calls) std::printf(" (%d, %d)", c.first, c.second);
        std::printf("\n");
        ++bad;
      }
    }
    std::printf("%s kind %2d (%s) over %zu widths\n", bad ? "FAIL" : "ok  ", kind, known ? "known" : "unknown", widths.size());
    failures += bad;
  }
  int bad = 0;
  for (int n = 0; n <= 16; ++n) {
    const int nc = gmb::pick_nc(n);
    Recorder r;
    gmb::with_kind_nc(GMB_EXPQUAD, nc, r);
    if (nc < n || r.calls.size() != 1 || r.calls[0].second != nc) {
      std::printf("     pick_nc(%d) = %d is not a width of the dispatcher that holds %d columns\n", n, nc, n);
      ++bad;
    }
  }
  std::printf("%s pick_nc(0 .. 16)\n", bad ? "FAIL" : "ok  ");
  failures += bad;
  std::printf("%s\n", failures ? "FAILED" : "all cases agree");
  return failures ? 1 : 0;
}
