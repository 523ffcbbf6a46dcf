// Chebyshev relaxation cycles for the 5-point Jacobi solver on a grid with
// fixed (Dirichlet) edges on all four sides. Host-only: shared by the kernel
// launchers, the solver and the _mxs_core bindings (the pure-Python twin is
// ops.chebyshev_cycle).
//
// One time-blocked pass of M levels becomes one M-point Chebyshev cycle of
// Richardson / Jacobi relaxation: level l runs
//   u' = u + w_l (A u - u) = (1 - w_l + w_l c_center) u + w_l c_neighbor (n + s + w + e)
// with its own weight w_l, i.e. the per-step form with a coefficient pair per
// level. Same stencil, reads, aprons and halo depth as the plain pass.
//
// On a W x H grid with fixed edges the eigenvalues of A are
//   c_center + 2 c_neighbor (cos(i pi / (W + 1)) + cos(j pi / (H + 1))),
// so those of I - A lie in [a, b] = [1 - c0 - 4 |c1| mu, 1 - c0 + 4 |c1| mu],
// mu = (cos(pi / (W + 1)) + cos(pi / (H + 1))) / 2. The cycle's error
// polynomial prod_l (1 - w_l x) is the degree-M Chebyshev polynomial of [a, b]
// scaled to 1 at 0: its roots are the Chebyshev points x_j of [a, b] and
// w_j = 1 / x_j. The product is the same in any order; the PREFIX products are
// not, and they bound how far the field strays inside a cycle. The roots are
// taken in Leja order (each next one maximises the product of its distances to
// those taken), which keeps the prefix maximum at 10^2 instead of 10^(M/2).
// `growth` is that maximum: max over l and x in [a, b] of |prod_{j <= l} (1 -
// w_j x)|. The field is only meaningful at cycle ends.
#pragma once

#include <cmath>
#include <limits>
#include <sstream>
#include <stdexcept>
#include <string>

namespace mxs {
namespace kernels {

// Levels a table holds: the deepest time block (kernels.hpp: kMaxTimeBlockDeep).
constexpr int kMaxLevels = 32;
// Samples of [a, b] the growth is taken over: the Chebyshev extrema
// (a + b) / 2 + (b - a) / 2 cos(pi k / K), k = 0..K, both endpoints included and
// dense towards them, where the prefix polynomials peak.
constexpr int kGrowthSamples = 2048;

// Cycle lengths the level-table kernels exist for (kernels.hpp:
// stencil5_tb_levels): fp32 20 and 24, fp64 12 and 16, the depths of the
// per-step pipeline passes.
constexpr bool relaxation_depth_supported(int elem_bytes, int M) {
  return elem_bytes == 4 ? (M == 20 || M == 24) : (M == 12 || M == 16);
}
// The cycle length an automatic time block takes (the larger depth; the
// smaller one only when the larger exceeds the tile).
constexpr int relaxation_auto_depth(int elem_bytes, long long tile_w, long long tile_h) {
  const int big = elem_bytes == 4 ? 24 : 16, small = elem_bytes == 4 ? 20 : 12;
  return (big <= tile_w && big <= tile_h) ? big : small;
}

struct LevelTable {
  int n = 0;
  double center[kMaxLevels] = {};
  double neighbor[kMaxLevels] = {};
  double growth = 0.0;
};

// [a, b] for the grid and the base coefficients.
struct RelaxSpectrum {
  double a = 0.0, b = 0.0;
};
inline RelaxSpectrum relaxation_spectrum(long long global_w, long long global_h, double c_center, double c_neighbor) {
  const double pi = 3.14159265358979323846;
  const double mu = (std::cos(pi / double(global_w + 1)) + std::cos(pi / double(global_h + 1))) / 2.0;
  const double r = 4.0 * std::fabs(c_neighbor) * mu;
  return {1.0 - c_center - r, 1.0 - c_center + r};
}

// The preconditions of a cycle on this grid (chebyshev_cycle's, without M).
inline void chebyshev_check(long long global_w, long long global_h, double c_center, double c_neighbor) {
  auto fail = [](const std::string& what) { throw std::invalid_argument("chebyshev_cycle: " + what); };
  if (global_w < 1 || global_h < 1) fail("the global grid must be non-empty");
  if (!(c_neighbor != 0.0)) fail("c_neighbor must not be 0 (the relaxation needs the neighbours)");
  const RelaxSpectrum sp = relaxation_spectrum(global_w, global_h, c_center, c_neighbor);
  if (!(sp.a > 0.0)) {
    std::ostringstream os;
    os << "the spectrum of I - A must be positive, but its lower end is " << sp.a << " (c_center " << c_center
       << ", c_neighbor " << c_neighbor << " on " << global_w << " x " << global_h
       << "): needs fixed edges on both axes and c_center + 4 |c_neighbor| mu < 1";
    fail(os.str());
  }
}

// The M-level cycle. Throws std::invalid_argument unless 1 <= M <= kMaxLevels,
// the grid is non-empty, c_neighbor != 0 and a > 0 (a periodic axis, or
// weights with c_center + 4 |c_neighbor| mu >= 1, give a <= 0: the operator is
// singular or not a contraction and the roots would reach 0).
inline LevelTable chebyshev_cycle(long long global_w, long long global_h, double c_center, double c_neighbor, int M) {
  if (M < 1 || M > kMaxLevels)
    throw std::invalid_argument("chebyshev_cycle: the cycle length must be in [1, " + std::to_string(kMaxLevels) + "], got " +
                                std::to_string(M));
  chebyshev_check(global_w, global_h, c_center, c_neighbor);
  const RelaxSpectrum sp = relaxation_spectrum(global_w, global_h, c_center, c_neighbor);
  const double pi = 3.14159265358979323846;
  const double mid = (sp.a + sp.b) / 2.0, half = (sp.b - sp.a) / 2.0;
  double root[kMaxLevels];
  for (int j = 0; j < M; ++j) root[j] = mid + half * std::cos(pi * double(2 * j + 1) / double(2 * M));
  // Leja order. The roots descend with j and are all positive, so root[0] has
  // the largest modulus. Mirror roots tie up to rounding: a candidate has to
  // beat the best by more than 1e-12 relative, so ties go to the lower j on
  // every platform.
  int order[kMaxLevels];
  bool taken[kMaxLevels] = {};
  order[0] = 0;
  taken[0] = true;
  for (int l = 1; l < M; ++l) {
    int best = -1;
    double best_p = 0.0;
    for (int k = 0; k < M; ++k) {
      if (taken[k]) continue;
      double p = 1.0;
      for (int q = 0; q < l; ++q) p *= std::fabs(root[k] - root[order[q]]);
      if (best < 0 || p > best_p * (1.0 + 1e-12)) {
        best = k;
        best_p = p;
      }
    }
    order[l] = best;
    taken[best] = true;
  }
  LevelTable t;
  t.n = M;
  double omega[kMaxLevels];
  for (int l = 0; l < M; ++l) {
    omega[l] = 1.0 / root[order[l]];
    t.center[l] = 1.0 - omega[l] + omega[l] * c_center;
    t.neighbor[l] = omega[l] * c_neighbor;
  }
  for (int k = 0; k <= kGrowthSamples; ++k) {
    const double x = mid + half * std::cos(pi * double(k) / double(kGrowthSamples));
    double p = 1.0;
    for (int l = 0; l < M; ++l) {
      p *= 1.0 - omega[l] * x;
      if (std::fabs(p) > t.growth) t.growth = std::fabs(p);
    }
  }
  return t;
}

// The weight of level l (c_neighbor: the base coefficient the table was made with).
inline double relaxation_omega(const LevelTable& t, double c_neighbor, int l) { return t.neighbor[l] / c_neighbor; }

// The range guard of a cycle in element type T (in the spirit of
// fast_form_verdict): inside a cycle the field strays by up to growth x max|u|
// (the held boundary ring counts in max|u|), which must stay below max(T) / 4.
template <typename T>
inline bool relaxation_range_ok(const LevelTable& t, double absmax) {
  return std::isfinite(absmax) && t.growth * absmax < double(std::numeric_limits<T>::max()) / 4.0;
}

}  // namespace kernels
}  // namespace mxs
