// Geometric multigrid for the fixed-edge Poisson solve u = A u + g,
// A u = c0 u + c1 (n + s + w + e) on a W x H core with Dirichlet values in a
// ghost ring of depth 1 (docs/ARCHITECTURE.md "Multigrid"). Host-only: the level
// planner and the sweep tables, shared by the kernel launchers, the native
// solver and the _mxs_core bindings (the pure-Python twin is ops.multigrid).
//
// Levels: vertex-centred coarsening n_c = (n - 1) / 2, coarse (I, J) on fine
// (2 I + 1, 2 J + 1), both axes together while both sides are odd, both >= 3
// and max(w, h) > kMgCoarsenAbove. The coarsest grid is solved by one workgroup
// in LDS, so both its sides must be <= kMgCoarsestMax.
//
// With c0 + 4 c1 = 1 (the pure Laplace operator) every level runs the same
// (c0, c1) and the coarse right-hand side is 4 R r (R: full weighting).
#pragma once

#include <cmath>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "mxs/kernels/relaxation.hpp"

namespace mxs {
namespace kernels {

constexpr long long kMgCoarsenAbove = 31;  // coarsen while max(w, h) is above this
constexpr long long kMgCoarsestMax = 63;   // sides the one-workgroup coarse solve holds
constexpr int kMgMaxSmooth = 4;            // nu_pre, nu_post in 1..4
constexpr int kMgCoarseLevels = 32;        // the coarse solve's Chebyshev cycle
constexpr int kMgMaxCoarseRepeats = 4096;

struct MgLevel {
  long long width = 0, height = 0;
};

inline bool mg_can_coarsen(long long w, long long h) {
  return w % 2 == 1 && h % 2 == 1 && w >= 3 && h >= 3 && (w > h ? w : h) > kMgCoarsenAbove;
}

// The sizes m 2^k - 1 (m <= 64) next to n on either side: the sides that
// coarsen down to at most kMgCoarsestMax on their own.
inline void mg_nearest_sizes(long long n, long long* below, long long* above) {
  long long p = 1;
  while ((n + 1) > 64 * p) p *= 2;
  *below = (n + 1) / p * p - 1;
  if (*below < 1) *below = 1;
  *above = ((n + 1) / p + 1) * p - 1;
}

// Finest level first. Throws std::invalid_argument when the grid is empty or
// the coarsening stops above kMgCoarsestMax.
inline std::vector<MgLevel> mg_plan_levels(long long w, long long h) {
  if (w < 1 || h < 1) throw std::invalid_argument("multigrid: the grid must be non-empty");
  std::vector<MgLevel> lv;
  lv.push_back({w, h});
  while (mg_can_coarsen(lv.back().width, lv.back().height))
    lv.push_back({(lv.back().width - 1) / 2, (lv.back().height - 1) / 2});
  const MgLevel c = lv.back();
  if (c.width > kMgCoarsestMax || c.height > kMgCoarsestMax) {
    long long wl, wu, hl, hu;
    mg_nearest_sizes(w, &wl, &wu);
    mg_nearest_sizes(h, &hl, &hu);
    std::ostringstream os;
    os << "multigrid: " << w << " x " << h << " does not coarsen: vertex-centred coarsening (n - 1) / 2 of both axes "
       << "together stops at " << c.width << " x " << c.height << " after " << lv.size() - 1
       << " steps (a side became even or fell below 3), and the coarsest grid must be at most " << kMgCoarsestMax
       << " on both sides. Sides m * 2^k - 1 with m <= 64 and the same k on both axes work (2047, 4095, 6143, 8191, "
       << "...); nearest to this grid: width " << wl << " or " << wu << ", height " << hl << " or " << hu;
    throw std::invalid_argument(os.str());
  }
  return lv;
}

// The operator every level shares: the pure Laplace weights.
inline void mg_check_operator(double c0, double c1) {
  if (!(std::fabs(c0 + 4.0 * c1 - 1.0) <= 1e-12) || !(c1 > 0.0)) {
    std::ostringstream os;
    os.precision(17);
    os << "multigrid: needs the pure Laplace operator, |c_center + 4 c_neighbor - 1| <= 1e-12 with c_neighbor > 0 "
       << "(then every level runs the same weights); got c_center " << c0 << ", c_neighbor " << c1;
    throw std::invalid_argument(os.str());
  }
}

// Sweep l of a table: x' = fma(neighbor[l], (n + s) + (w + e), center[l] * c),
// then + T(weight[l]) * g (the product rounded, then the sum).
struct MgSweepTable {
  int n = 0;
  double center[kMaxLevels] = {};
  double neighbor[kMaxLevels] = {};
  double weight[kMaxLevels] = {};
};

// `sweeps` damped-Jacobi sweeps: w = omega / (1 - c0), center = 1 - w + w c0,
// neighbor = w c1 (the default weights with omega 0.8: exactly (0.2, 0.2, 1)).
inline MgSweepTable mg_smoother_table(double c0, double c1, double omega, int sweeps) {
  if (sweeps < 1 || sweeps > kMgMaxSmooth)
    throw std::invalid_argument("multigrid: nu_pre and nu_post must be in 1.." + std::to_string(kMgMaxSmooth) +
                                ", got " + std::to_string(sweeps));
  if (!(omega > 0.0) || !(omega <= 1.0))
    throw std::invalid_argument("multigrid: smoother_omega must be in (0, 1]");
  MgSweepTable t;
  t.n = sweeps;
  const double w = omega / (1.0 - c0);
  for (int l = 0; l < sweeps; ++l) {
    t.weight[l] = w;
    t.center[l] = 1.0 - w + w * c0;
    t.neighbor[l] = w * c1;
  }
  return t;
}

// The coarsest level's solve: the 32-level Leja-ordered Chebyshev cycle of its
// grid, repeated `repeats` times from e = 0. The weight of level l is
// relaxation_omega(); `rho` is the cycle's error bound, the maximum of |prod_l
// (1 - w_l x)| over the kGrowthSamples + 1 Chebyshev extrema of the spectrum,
// and `repeats` the smallest R with rho^R <= coarse_reduction.
struct MgCoarsePlan {
  MgSweepTable table;
  int repeats = 1;
  double rho = 0.0;
};
inline MgCoarsePlan mg_coarse_plan(long long w, long long h, double c0, double c1, double coarse_reduction) {
  if (!(coarse_reduction > 0.0) || !(coarse_reduction < 1.0))
    throw std::invalid_argument("multigrid: coarse_reduction must be in (0, 1)");
  const LevelTable t = chebyshev_cycle(w, h, c0, c1, kMgCoarseLevels);
  MgCoarsePlan p;
  p.table.n = t.n;
  for (int l = 0; l < t.n; ++l) {
    p.table.center[l] = t.center[l];
    p.table.neighbor[l] = t.neighbor[l];
    p.table.weight[l] = relaxation_omega(t, c1, l);
  }
  const RelaxSpectrum sp = relaxation_spectrum(w, h, c0, c1);
  const double pi = 3.14159265358979323846;
  const double mid = (sp.a + sp.b) / 2.0, half = (sp.b - sp.a) / 2.0;
  for (int k = 0; k <= kGrowthSamples; ++k) {
    const double x = mid + half * std::cos(pi * double(k) / double(kGrowthSamples));
    double q = 1.0;
    for (int l = 0; l < t.n; ++l) q *= 1.0 - p.table.weight[l] * x;
    if (std::fabs(q) > p.rho) p.rho = std::fabs(q);
  }
  if (!(p.rho < 1.0)) throw std::invalid_argument("multigrid: the coarse cycle does not contract");
  double r = p.rho;
  while (r > coarse_reduction) {
    r *= p.rho;
    ++p.repeats;
    if (p.repeats > kMgMaxCoarseRepeats) throw std::invalid_argument("multigrid: the coarse solve needs too many cycles");
  }
  return p;
}

}  // namespace kernels
}  // namespace mxs
