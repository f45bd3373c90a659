// workspace_sizes.hpp -- the constants the engine's workspaces are sized by (workspaces.hpp).  The headers whose kernels they belong
// to include this one: there is one copy of each.  No HIP and no engine types (tools/workspace_budget_check.cpp reads it on the host).
#pragma once

#if defined(__HIPCC__)
#define GMB_HOST_DEVICE __host__ __device__
#else
#define GMB_HOST_DEVICE  // a host-only build: the qualifiers mean nothing there
#endif

namespace gmb {

// covariance.hpp
constexpr int MAX_TABS = 5;     // GMB_MAX_COREG + output coregion
constexpr int MAX_LIN = 8;      // GMB_MAX_LIN
constexpr int XS_ROWS = 17;     // rows of a prepared point set's xs: 16 scaled continuous dims at most + the squared norm
constexpr int RED_CHUNK = 256;  // training rows per chunk of the posterior reductions' first stage
// group_average.hpp
constexpr int GA_ROWS = 128;    // groups per row block of the Q pass (the leading dimension of R)
// predict_terms.hpp
constexpr int TG_MAX_TERMS = 5;  // 1 + GMB_MAX_COREG: 5 means + 15 products = 20 f64 accumulators per thread
// entries per test point and chunk: NT means, then the packed lower triangle (row p = t (t + 1) / 2 + u, u <= t)
GMB_HOST_DEVICE constexpr int tg_entries(int nt) { return nt + nt * (nt + 1) / 2; }

}  // namespace gmb
