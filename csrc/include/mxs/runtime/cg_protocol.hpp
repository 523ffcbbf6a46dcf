// The host protocol of a CG-family solve, once: CgSolver and PcgSolver both run
// cg_drive (docs/ARCHITECTURE.md "The CG host driver"). Host-only, no device
// needed: tests/cpp/unit_tests.cpp drives it with scripted callables.
//
// The device decides when an iteration stops, on the recursive residual. The
// host starts a run, steps it block by block until the status leaves
// kCgRunning, and confirms a reported convergence on the true residual: above
// tol the solve restarts from the field as it stands, with the iterations
// already spent counted, and after kCgMaxRestarts restarts it ends "stalled"
// (the element type's floor).
#pragma once

#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "mxs/core/config.hpp"
#include "mxs/kernels/cg.hpp"

namespace mxs {

struct CgResidual {
  double linf = 0.0, l2 = 0.0;
  index_t cells = 0;
};

struct CgSolve {
  bool converged = false;
  int iterations = 0;
  double residual = 0.0;  // the true residual in the chosen norm
  std::string reason, norm;
  int restarts = 0;
  struct Check {
    int iteration;
    double linf, l2;  // of the recursive residual, as the device holds it
  };
  std::vector<Check> history;
};

constexpr int kCgMaxRestarts = 3;

// What cg_drive reads of a device scalar block (CgScalars or PcgScalars).
struct CgProgress {
  int status = kernels::kCgRunning;
  int iteration = 0;  // of the current run
  double rr = 0.0, linf = 0.0;
};

// who: the prefix of the argument errors ("conjugate gradients").
//   start(tol, remaining, norm_id) -> CgProgress   upload the controls, launch the start kernel, read the scalars
//   step() -> CgProgress                           one block of `block` iterations, read the scalars
//   true_residual() -> CgResidual
// `block` (check_every) is only checked here: the callables own the launches.
template <typename Start, typename Step, typename TrueResidual>
CgSolve cg_drive(const char* who, double tol, int max_iters, const std::string& norm, int block, Start&& start,
                 Step&& step, TrueResidual&& true_residual) {
  if (norm != "linf" && norm != "l2")
    throw std::invalid_argument(std::string(who) + ": norm must be 'linf' or 'l2', got '" + norm + "'");
  if (!(tol >= 0.0) || max_iters < 0 || block < 1)
    throw std::invalid_argument(std::string(who) + ": solve needs tol >= 0, max_iters >= 0 and check_every >= 1");
  const int norm_id = norm == "linf" ? kernels::kCgNormLinf : kernels::kCgNormL2;
  CgSolve out;
  out.norm = norm;
  int remaining = max_iters;
  bool have_true = false;
  for (;;) {  // one run from the start kernel
    CgProgress sc = start(tol, remaining, norm_id);
    out.history.push_back({out.iterations, sc.linf, std::sqrt(sc.rr)});
    while (sc.status == kernels::kCgRunning) {
      sc = step();
      out.history.push_back({out.iterations + sc.iteration, sc.linf, std::sqrt(sc.rr)});
    }
    out.iterations += sc.iteration;
    remaining -= sc.iteration;
    if (sc.status == kernels::kCgConverged) {
      const CgResidual t = true_residual();
      out.residual = norm_id == kernels::kCgNormLinf ? t.linf : t.l2;
      have_true = true;
      if (!std::isfinite(out.residual) || !std::isfinite(t.linf)) {
        out.reason = "non-finite residual";
      } else if (out.residual <= tol) {
        out.converged = true;
        out.reason = "converged: " + norm + " residual <= tol";
      } else if (out.restarts >= kCgMaxRestarts) {
        out.reason = "stalled";
      } else if (remaining <= 0) {
        out.reason = "max_iters reached";
      } else {
        ++out.restarts;  // the recursive residual drifted from the true one: start again from u
        continue;
      }
    } else if (sc.status == kernels::kCgMaxIters) {
      out.reason = "max_iters reached";
    } else {
      out.reason = std::isfinite(sc.rr) && std::isfinite(sc.linf) ? "breakdown" : "non-finite residual";
    }
    break;
  }
  if (!have_true) {
    const CgResidual t = true_residual();
    out.residual = norm_id == kernels::kCgNormLinf ? t.linf : t.l2;
  }
  return out;
}

}  // namespace mxs
