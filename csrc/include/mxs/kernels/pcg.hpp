// Multigrid-preconditioned conjugate gradients for the fixed-edge solve
// u = A u + g on any W x H core (docs/ARCHITECTURE.md "Preconditioned CG").
// Host-only: the level plan of the preconditioner, its coarse solve plan and
// the layout of the device scalar block, shared by the kernel launchers, the
// native solver and the _mxs_core bindings (the pure-Python twin is ops.pcg).
//
// The preconditioner is ONE V-cycle from e = 0 on L e = r. It does not have to
// converge on its own (on even sides it does not); it only has to be a fixed
// symmetric positive-definite operator, which nu_pre == nu_post, the symmetric
// smoother and P = R^T / 4 give.
//
// Levels: both axes coarsen together with n_c = floor(n / 2), coarse (I, J) on
// fine (2 I + 1, 2 J + 1), while max(w, h) > kMgCoarsenAbove and min(w, h) >= 2.
// On an odd side that is multigrid.hpp's (n - 1) / 2. On an even side the last
// coarse point sits on the last fine point, one fine spacing (half a coarse
// spacing) from the edge: the coarse level then carries a REFLECT flag for that
// side, and the ghost cell beyond its last core row (column) reads as the
// negated last core cell: a Dirichlet zero half a spacing away. The negation is
// exact and the coarse operator stays symmetric (a diagonal shift of + c1).
// Near sides and non-reflecting far sides keep a ring of 0; level 0 never
// reflects.
//
// Screened operators: with sigma = 1 - c0 - 4 c1 >= 0 level k runs (c0_k, c1),
// c0_k = 1 - 4 c1 - 4^k sigma = c0 - (4^k - 1) sigma, and the coarse right-hand
// side stays 4 R r. |sigma| <= 1e-12 (mg_check_operator's bound) counts as 0, so
// the pure Laplace weights run the same doubles on every level.
//
// Neumann sides (cg.hpp's GhostSides; docs/ARCHITECTURE.md "Neumann sides"):
// every level carries four ghost codes. Level 0 has the solve's (ring or
// mirror). Near sides (top, left) of a coarse level inherit the kind. A far side
// (bottom, right) is a mirror on every level when the finest level's is,
// whatever the parity; otherwise the rule above: reflect under an even parent,
// else ring. reflect_rows is bottom == -1 and reflect_cols is right == -1.
#pragma once

#include <cmath>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "mxs/kernels/cg.hpp"
#include "mxs/kernels/multigrid.hpp"
#include "mxs/kernels/relaxation.hpp"

namespace mxs {
namespace kernels {

// The device block the PCG kernels share (CgScalars' rules: every workgroup
// reads status, and alpha or beta, once at entry; only the last workgroup of a
// launch writes). Who writes what:
//   pcg_start            rr, linf, rz = 0, pq = 0, alpha = 0, beta = 0, iteration = 0, status
//   mgp_smooth (dot)     rz, beta = rz' / rz (0 while iteration == 0)
//   pcg_apply            pq, alpha = rz / pq (or status = kCgBreakdown)
//   pcg_update           rr, linf, ++iteration, status
struct PcgScalars {
  double rr;     // sum r^2 of the recursive residual
  double rz;     // sum r z, z = M r
  double pq;     // sum p (L p)
  double alpha;  // rz / pq
  double beta;   // rz' / rz
  double linf;   // max |r|
  double tol;    // host: the stopping threshold of the chosen norm
  int iteration;
  int max_iters;  // host
  int norm;       // host: kCgNormLinf or kCgNormL2
  int status;     // CgStatus
};
static_assert(sizeof(PcgScalars) == 72, "PcgScalars: 7 doubles and 4 ints, no padding");

struct PcgLevel {
  long long width = 0, height = 0;
  bool reflect_rows = false;  // the ghost row `height` reads as minus row height - 1
  bool reflect_cols = false;  // the ghost column `width` reads as minus column width - 1
  double c0 = 0.0;            // c_center of this level
  GhostSides sides;           // the four ghost codes; bottom == -1 <=> reflect_rows, right == -1 <=> reflect_cols
};

// A level from its flags and codes: a far code of 0 under a set flag becomes -1.
inline PcgLevel pcg_level_of(long long w, long long h, bool reflect_rows, bool reflect_cols, double c0,
                             GhostSides sides = {}) {
  if (reflect_rows && sides.bottom == kGhostRing) sides.bottom = kGhostReflect;
  if (reflect_cols && sides.right == kGhostRing) sides.right = kGhostReflect;
  PcgLevel l;
  l.width = w;
  l.height = h;
  l.reflect_rows = sides.bottom == kGhostReflect;
  l.reflect_cols = sides.right == kGhostReflect;
  l.c0 = c0;
  l.sides = sides;
  return l;
}

inline bool pcg_can_coarsen(long long w, long long h) {
  return (w > h ? w : h) > kMgCoarsenAbove && (w < h ? w : h) >= 2;
}

// Finest level first. Throws std::invalid_argument when the grid is empty, the
// weights are not CG's or the coarsening stops above kMgCoarsestMax (only very
// thin grids do; they are well conditioned).
inline std::vector<PcgLevel> pcg_plan_levels(long long w, long long h, double c0, double c1, GhostSides sides = {}) {
  if (w < 1 || h < 1) throw std::invalid_argument("preconditioned CG: the grid must be non-empty");
  cg_check_sides(c0, c1, sides);
  double sigma = 1.0 - c0 - 4.0 * c1;
  if (std::fabs(sigma) <= 1e-12) sigma = 0.0;
  std::vector<PcgLevel> lv;
  lv.push_back(pcg_level_of(w, h, false, false, c0, sides));
  double scale = 1.0;  // 4^k
  while (pcg_can_coarsen(lv.back().width, lv.back().height)) {
    const PcgLevel f = lv.back();
    scale *= 4.0;
    const bool mirror_rows = sides.bottom == kGhostMirror, mirror_cols = sides.right == kGhostMirror;
    lv.push_back(pcg_level_of(f.width / 2, f.height / 2, !mirror_rows && f.height % 2 == 0,
                              !mirror_cols && f.width % 2 == 0, c0 - (scale - 1.0) * sigma,
                              GhostSides{sides.top, mirror_rows ? kGhostMirror : kGhostRing, sides.left,
                                         mirror_cols ? kGhostMirror : kGhostRing}));
  }
  const PcgLevel c = lv.back();
  if (c.width > kMgCoarsestMax || c.height > kMgCoarsestMax) {
    std::ostringstream os;
    os << "preconditioned CG: " << w << " x " << h << " is too thin to coarsen: halving both axes together stops at "
       << c.width << " x " << c.height << " after " << lv.size() - 1 << " steps (a side fell below 2), and the coarsest "
       << "grid must be at most " << kMgCoarsestMax << " on both sides. Such grids are well conditioned: use "
       << "ConjugateGradient2D";
    throw std::invalid_argument(os.str());
  }
  return lv;
}

// chebyshev_cycle on a given interval [a, b], 0 < a < b: the same roots, the same
// Leja order and tie rule, the same tables (relaxation.hpp). For operators whose
// spectrum relaxation_spectrum does not bound.
inline LevelTable chebyshev_cycle_interval(double a, double b, double c_center, double c_neighbor, int M) {
  if (M < 1 || M > kMaxLevels)
    throw std::invalid_argument("chebyshev_cycle_interval: the cycle length must be in [1, " +
                                std::to_string(kMaxLevels) + "], got " + std::to_string(M));
  if (!(a > 0.0) || !(b > a) || !std::isfinite(b))
    throw std::invalid_argument("chebyshev_cycle_interval: needs 0 < a < b");
  if (!(c_neighbor != 0.0)) throw std::invalid_argument("chebyshev_cycle_interval: c_neighbor must not be 0");
  const double pi = 3.14159265358979323846;
  const double mid = (a + b) / 2.0, half = (b - a) / 2.0;
  double root[kMaxLevels];
  for (int j = 0; j < M; ++j) root[j] = mid + half * std::cos(pi * double(2 * j + 1) / double(2 * M));
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

// The interval the coarse solve of a level is built on. Without a reflecting
// side it is relaxation_spectrum's. A reflecting side adds + c1 on part of the
// diagonal, a positive semi-definite term: the lower end still holds, and the
// upper end becomes the Gershgorin bound 1 - c0 + 4 c1, which reflecting rows
// still meet (diagonal 1 - c0 + c1, three neighbours of weight c1 at most).
//
// A level with a mirror side: a = 1 - c0 - c1 (mu_x + mu_y) with mu the largest
// eigenvalue of the 1-D neighbour matrix of n cells under its two end codes
// (pcg_axis_mu: exact, the operator is a Kronecker sum), b the Gershgorin bound.
inline double pcg_axis_mu(long long n, int s, int t) {
  const double pi = 3.14159265358979323846;
  const int mirrors = (s == kGhostMirror) + (t == kGhostMirror), reflects = (s == kGhostReflect) + (t == kGhostReflect);
  const double dn = double(n);
  if (mirrors == 0 && reflects == 0) return 2.0 * std::cos(pi / (dn + 1.0));
  if (mirrors == 1 && reflects == 0) return 2.0 * std::cos(pi / (2.0 * dn + 1.0));
  if (mirrors == 2) return 2.0;
  if (mirrors == 0 && reflects == 1) return 2.0 * std::cos(2.0 * pi / (2.0 * dn + 1.0));
  if (mirrors == 1 && reflects == 1) return 2.0 * std::cos(pi / (2.0 * dn));
  return 2.0 * std::cos(pi / dn);  // reflect, reflect
}

inline RelaxSpectrum pcg_coarse_interval(const PcgLevel& l, double c1) {
  if (l.sides.any_mirror()) {
    const double mu = pcg_axis_mu(l.width, l.sides.left, l.sides.right) + pcg_axis_mu(l.height, l.sides.top, l.sides.bottom);
    return {1.0 - l.c0 - c1 * mu, 1.0 - l.c0 + 4.0 * c1};
  }
  RelaxSpectrum sp = relaxation_spectrum(l.width, l.height, l.c0, c1);
  if (l.reflect_rows || l.reflect_cols) sp.b = 1.0 - l.c0 + 4.0 * c1;
  return sp;
}

// The coarsest level's solve. A level without a reflecting side takes
// mg_coarse_plan as it is; a reflecting one the 32-point cycle of
// pcg_coarse_interval (a Chebyshev polynomial grows outside its interval, and a
// reflecting level has eigenvalues above relaxation_spectrum's upper end).
inline MgCoarsePlan pcg_coarse_plan(const PcgLevel& l, double c1, double coarse_reduction) {
  if (!l.reflect_rows && !l.reflect_cols && !l.sides.any_mirror())
    return mg_coarse_plan(l.width, l.height, l.c0, c1, coarse_reduction);
  if (!(coarse_reduction > 0.0) || !(coarse_reduction < 1.0))
    throw std::invalid_argument("preconditioned CG: coarse_reduction must be in (0, 1)");
  const RelaxSpectrum sp = pcg_coarse_interval(l, c1);
  if (!(sp.a > 0.0)) {
    std::ostringstream os;
    os.precision(17);
    os << "preconditioned CG: the coarsest level's operator is singular (lower spectrum end " << sp.a << "): with all "
       << "four sides Neumann the operator needs screening (c_center + 4 c_neighbor < 1), or one side held fixed";
    throw std::invalid_argument(os.str());
  }
  const LevelTable t = chebyshev_cycle_interval(sp.a, sp.b, l.c0, c1, kMgCoarseLevels);
  MgCoarsePlan p;
  p.table.n = t.n;
  for (int k = 0; k < t.n; ++k) {
    p.table.center[k] = t.center[k];
    p.table.neighbor[k] = t.neighbor[k];
    p.table.weight[k] = relaxation_omega(t, c1, k);
  }
  const double pi = 3.14159265358979323846;
  const double mid = (sp.a + sp.b) / 2.0, half = (sp.b - sp.a) / 2.0;
  for (int k = 0; k <= kGrowthSamples; ++k) {
    const double x = mid + half * std::cos(pi * double(k) / double(kGrowthSamples));
    double q = 1.0;
    for (int j = 0; j < t.n; ++j) q *= 1.0 - p.table.weight[j] * x;
    if (std::fabs(q) > p.rho) p.rho = std::fabs(q);
  }
  if (!(p.rho < 1.0)) throw std::invalid_argument("preconditioned CG: the coarse cycle does not contract");
  double r = p.rho;
  while (r > coarse_reduction) {
    r *= p.rho;
    ++p.repeats;
    if (p.repeats > kMgMaxCoarseRepeats)
      throw std::invalid_argument(
          l.sides.all_mirror()
              ? "preconditioned CG: the coarse solve needs too many cycles: with all four sides Neumann and so little "
                "screening the coarsest operator is nearly singular (constants are almost in its null space); hold one "
                "side fixed or use a larger 1 - c_center - 4 c_neighbor"
              : "preconditioned CG: the coarse solve needs too many cycles");
  }
  return p;
}

}  // namespace kernels
}  // namespace mxs
