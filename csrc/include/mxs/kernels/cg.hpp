// Conjugate gradients for L u = b with L v = (1 - c0) v - c1 (n + s + w + e) on
// a W x H core with Dirichlet values in a ghost ring of depth 1
// (docs/ARCHITECTURE.md "Conjugate gradients"). Host-only: the operator check
// and the layout of the device scalar block, shared by the kernel launchers,
// the native solver and the _mxs_core bindings.
//
// The ring is folded into the right-hand side: the residual of the system is
// the project's own r = (A u + g) - u, A u = c0 u + c1 (n + s + w + e), so
// L e = r for the error e of u. L is symmetric; with c1 > 0 and c0 + 4 c1 <= 1
// its spectrum lies in [1 - c0 - 4 c1 mu, 1 - c0 + 4 c1 mu], mu < 1
// (relaxation_spectrum), so it is positive definite on any grid.
#pragma once

#include <cmath>
#include <sstream>
#include <stdexcept>

namespace mxs {
namespace kernels {

// The device block the three kernels share. No launch writes a member that
// other workgroups of the same launch read: every workgroup reads status (and
// alpha or beta) once at entry, only the last workgroup of a launch writes.
struct CgScalars {
  double rr;     // sum r^2 of the recursive residual
  double pq;     // sum p (L p)
  double alpha;  // rr / pq
  double beta;   // rr' / rr
  double linf;   // max |r|
  double tol;    // host: the stopping threshold of the chosen norm
  int iteration;
  int max_iters;  // host
  int norm;       // host: kCgNormLinf or kCgNormL2
  int status;     // CgStatus
};
static_assert(sizeof(CgScalars) == 64, "CgScalars: 6 doubles and 4 ints, no padding");

constexpr int kCgNormLinf = 0;
constexpr int kCgNormL2 = 1;
enum CgStatus : int { kCgRunning = 0, kCgConverged = 1, kCgMaxIters = 2, kCgBreakdown = 3 };

// Admissible weights: c1 > 0 and c0 + 4 c1 <= 1 (then L is symmetric positive
// definite); the pure Laplace weights and every screened operator below them.
inline void cg_check_operator(double c0, double c1) {
  if (!(c1 > 0.0) || !(c0 + 4.0 * c1 <= 1.0 + 1e-12) || !std::isfinite(c0)) {
    std::ostringstream os;
    os.precision(17);
    os << "conjugate gradients: needs c_neighbor > 0 and c_center + 4 c_neighbor <= 1 (then (1 - c_center) v - "
       << "c_neighbor (n + s + w + e) is symmetric positive definite); got c_center " << c0 << ", c_neighbor " << c1;
    throw std::invalid_argument(os.str());
  }
}

}  // namespace kernels
}  // namespace mxs
