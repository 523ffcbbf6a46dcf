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
#include <string>
#include <utility>

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

// What the ghost cell beyond each side of the core reads as (docs/ARCHITECTURE.md
// "Neumann sides"). Sides are named as set_boundary names them: top is row -1,
// bottom row H, left column -1, right column W.
//   kGhostRing     the ring cell itself: a Dirichlet value (the default)
//   kGhostMirror   edge + ring: a Neumann side, the ring cell holding the
//                  prescribed outward difference d = u_ghost - u_edge (0:
//                  insulated). Where the operator acts on a direction or an
//                  error (cg_apply, the preconditioner) d is 0 and the ghost is
//                  the edge cell itself.
//   kGhostReflect  minus the edge cell, the ring never read: the far side of a
//                  coarse preconditioner level under an even parent (pcg.hpp).
constexpr int kGhostRing = 0;
constexpr int kGhostMirror = 1;
constexpr int kGhostReflect = -1;

struct GhostSides {
  int top = kGhostRing, bottom = kGhostRing, left = kGhostRing, right = kGhostRing;
  bool any_mirror() const {
    return top == kGhostMirror || bottom == kGhostMirror || left == kGhostMirror || right == kGhostMirror;
  }
  bool all_mirror() const {
    return top == kGhostMirror && bottom == kGhostMirror && left == kGhostMirror && right == kGhostMirror;
  }
  bool all_ring() const { return top == 0 && bottom == 0 && left == 0 && right == 0; }
};

// The Neumann sides of a solve by name; unknown and repeated names throw.
template <typename Names>
inline GhostSides ghost_sides_of(const Names& neumann) {
  GhostSides s;
  for (const std::string& n : neumann) {
    int* side = n == "top" ? &s.top : n == "bottom" ? &s.bottom : n == "left" ? &s.left : n == "right" ? &s.right : nullptr;
    if (side == nullptr)
      throw std::invalid_argument("neumann: unknown side '" + n + "' (the sides are top, bottom, left and right)");
    if (*side != kGhostRing) throw std::invalid_argument("neumann: side '" + n + "' is named twice");
    *side = kGhostMirror;
  }
  return s;
}

inline std::string ghost_sides_names(const GhostSides& s) {
  std::string out;
  const std::pair<const char*, int> all[] = {{"top", s.top}, {"bottom", s.bottom}, {"left", s.left}, {"right", s.right}};
  for (const auto& p : all)
    if (p.second == kGhostMirror) out += (out.empty() ? "" : ", ") + std::string(p.first);
  return out;
}

// cg_check_operator plus the one rule the sides add: with all four sides
// Neumann and sigma = 1 - c0 - 4 c1 = 0 the operator is singular (constants are
// its null space).
inline void cg_check_sides(double c0, double c1, const GhostSides& s) {
  cg_check_operator(c0, c1);
  for (int code : {s.top, s.bottom, s.left, s.right})
    if (code != kGhostRing && code != kGhostMirror)
      throw std::invalid_argument("neumann: a side of the solve is dirichlet (0) or neumann (+1)");
  if (s.all_mirror() && std::fabs(1.0 - c0 - 4.0 * c1) <= 1e-12) {
    std::ostringstream os;
    os.precision(17);
    os << "neumann: with all four sides Neumann and c_center + 4 c_neighbor = 1 (got c_center " << c0 << ", c_neighbor "
       << c1 << ") the operator is singular: constants are its null space. Hold one side fixed (Dirichlet), or use a "
       << "screened operator (c_center + 4 c_neighbor < 1)";
    throw std::invalid_argument(os.str());
  }
}

}  // namespace kernels
}  // namespace mxs
