// PcgSolver<T>: conjugate gradients preconditioned by one any-size V-cycle, for
// the fixed-edge solve u = A u + g on one GPU, any W x H the level plan accepts
// and any admissible weights (mxs/kernels/pcg.hpp, docs/ARCHITECTURE.md
// "Preconditioned CG").
//
// It owns the tiles u, g, r, q and a p ping-pong pair of TileGeom::aligned(w, h,
// 1, 1), the level tiles of the preconditioner, the device scalar block and one
// stream. The preconditioner's finest level has the residual r as its source,
// z as its output and a ring of 0. One iteration is the V-cycle (its last
// launch leaves rz and beta), pcg_apply, pcg_update. solve() follows CgSolver's
// host protocol: pcg_start, blocks of iterations, a pinned read of the scalar
// block; the device decides when the iteration stops, so the host's cadence
// cannot change a bit of the result. With cfg.graph a block is one linear
// captured hipGraph (one stream, no branches, an even number of iterations so
// the p ping-pong closes); eager launches give the same bits. A reported
// convergence is confirmed on the true residual, else a restart (at most
// kCgMaxRestarts, then "stalled").
//
// cfg.neumann names the Neumann sides: pcg_start, pcg_apply and the true
// residual follow CgSolver, and every level of the preconditioner carries its
// ghost codes (mxs/kernels/pcg.hpp), mirrored transfers included.
#pragma once

#include <string>
#include <vector>

#include "mxs/kernels/kernels.hpp"
#include "mxs/runtime/cg_solver.hpp"
#include "mxs/runtime/hip_utils.hpp"

namespace mxs {

struct PcgConfig {
  index_t width = 0, height = 0;
  double c_center = 0.2, c_neighbor = 0.2;
  int nu = 2;  // nu_pre == nu_post: the preconditioner must be symmetric
  double smoother_omega = 0.8;
  double coarse_reduction = 1e-3;
  bool graph = true;
  std::vector<std::string> neumann;  // CgConfig::neumann: the Neumann sides by name
};

// The setters and getters, residual(), solve() (the same CgSolve record) and
// scalars() are CgSolverBase's.
template <typename T>
class PcgSolver : public CgSolverBase<T, kernels::PcgScalars> {
 public:
  explicit PcgSolver(const PcgConfig& cfg);

  const PcgConfig& config() const { return cfg_; }
  const std::vector<kernels::PcgLevel>& levels() const { return plan_; }
  int launches_per_iteration() const { return launches_; }
  std::string note() const override;

 private:
  struct Level {
    TileGeom geom;
    DeviceBuffer<T> u[2], g;  // level 0 has no g of its own: its source is r
    kernels::MgSweepTable smooth;
  };
  void enqueue_level(size_t k);
  void launch_start(bool into_scratch) override;
  void launch_heat_start(const kernels::HeatCoeffs& hc, const T* q) override;
  void enqueue_iterations(int n, int parity) override;

  PcgConfig cfg_;
  std::vector<kernels::PcgLevel> plan_;
  kernels::MgCoarsePlan coarse_;
  std::vector<Level> lv_;
  int launches_ = 0;
};

}  // namespace mxs
