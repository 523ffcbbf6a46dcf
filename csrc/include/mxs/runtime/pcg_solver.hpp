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

template <typename T>
class PcgSolver {
 public:
  using value_type = T;
  explicit PcgSolver(const PcgConfig& cfg);
  PcgSolver(const PcgSolver&) = delete;
  PcgSolver& operator=(const PcgSolver&) = delete;

  const PcgConfig& config() const { return cfg_; }
  const TileGeom& geom() const { return geom_; }
  const std::vector<kernels::PcgLevel>& levels() const { return plan_; }

  void set_boundary(const T* top, const T* bottom, const T* left, const T* right);
  void set_source(const T* tile);
  void set_field(const T* tile);
  void field(T* tile);
  CgResidual residual();
  // CgSolve: the same record (iterations, the true residual, reason, restarts, history).
  CgSolve solve(double tol, int max_iters, const std::string& norm, int check_every);
  kernels::PcgScalars scalars();
  std::string graph_status() const { return graph_status_; }
  int launches_per_iteration() const { return launches_; }
  std::string note() const;

 private:
  struct Level {
    TileGeom geom;
    DeviceBuffer<T> u[2], g;  // level 0 has no g of its own: its source is r
    kernels::MgSweepTable smooth;
  };
  void enqueue_level(size_t k);
  void enqueue_iterations(int n, int parity);
  bool capture(int iters);
  kernels::PcgScalars start(double tol, int max_iters, int norm);
  kernels::PcgScalars read_scalars();

  PcgConfig cfg_;
  kernels::GhostSides sides_;
  TileGeom geom_;
  std::vector<kernels::PcgLevel> plan_;
  kernels::MgCoarsePlan coarse_;
  std::vector<Level> lv_;
  DeviceBuffer<T> u_, g_, r_, q_, p_[2];
  DeviceBuffer<kernels::PcgScalars> scalars_, residual_scalars_;
  DeviceBuffer<double> partials_, residual_buf_;
  DeviceBuffer<unsigned> counter_, residual_counter_;
  PinnedBuffer<kernels::PcgScalars> scalars_host_;
  PinnedBuffer<double> residual_host_;
  Stream stream_;
  GraphExec graph_;
  int graph_iters_ = 0;
  int launches_ = 0;
  std::string graph_status_ = "off";
};

}  // namespace mxs
