// Implicit heat steps: the theta-scheme for u_t = kappa lap(u) + f as the
// project's own fixed-edge problem (docs/ARCHITECTURE.md "Implicit heat steps").
// Host-only: the coefficients, once, for the kernel launchers, the native
// solvers, the _mxs_core bindings and ops/heat.py.
//
// With lam = kappa dt / h^2 > 0, 0.5 <= theta <= 1 (1: backward Euler, 0.5:
// Crank-Nicolson) and D = 1 + 4 theta lam, one step u -> u' solves
//   u' = A u' + g,   A v = c1 (n + s + w + e),   c1 = theta lam / D   (c_center = 0)
//   g  = a u + b (n + s + w + e) + s q,
//   a  = (1 - 4 (1 - theta) lam) / D,  b = (1 - theta) lam / D,  s = 1 / D,  q = dt f.
// 4 c1 = 1 - 1 / D < 1: the operator is admissible and screened (sigma = 1 / D),
// so it is legal with four Neumann sides too. lambda_min(L) >= 1 / D, so the
// error of a step solved to a residual r is at most D ||r||_2.
#pragma once

#include <cmath>
#include <sstream>
#include <stdexcept>

namespace mxs {
namespace kernels {

struct HeatCoeffs {
  double c1 = 0.0;  // the solve's c_neighbor (its c_center is 0)
  double a = 0.0;   // g's weight of the centre
  double b = 0.0;   // g's weight of the four neighbours (0 for backward Euler)
  double s = 0.0;   // g's weight of the source q = dt f: 1 / D
};

inline HeatCoeffs heat_coefficients(double lam, double theta) {
  std::ostringstream os;
  os.precision(17);
  if (!std::isfinite(lam) || !std::isfinite(theta)) {
    os << "implicit heat step: lam and theta must be finite, got lam " << lam << ", theta " << theta;
    throw std::invalid_argument(os.str());
  }
  if (!(lam > 0.0)) {
    os << "implicit heat step: needs lam = kappa dt / h^2 > 0, got " << lam;
    throw std::invalid_argument(os.str());
  }
  if (theta < 0.5) {
    os << "implicit heat step: theta " << theta << " < 0.5 is only conditionally stable (it needs lam <= 1 / (4 (1 - 2 "
       << "theta))); this stepper takes 0.5 <= theta <= 1, the explicit stepper is Stencil2D";
    throw std::invalid_argument(os.str());
  }
  if (theta > 1.0) {
    os << "implicit heat step: needs 0.5 <= theta <= 1 (0.5: Crank-Nicolson, 1: backward Euler), got " << theta;
    throw std::invalid_argument(os.str());
  }
  const double D = 1.0 + 4.0 * theta * lam;
  HeatCoeffs h;
  h.c1 = theta * lam / D;
  h.a = (1.0 - 4.0 * (1.0 - theta) * lam) / D;
  h.b = (1.0 - theta) * lam / D;
  h.s = 1.0 / D;
  return h;
}

}  // namespace kernels
}  // namespace mxs
