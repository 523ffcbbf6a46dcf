// MultigridSolver<T>: geometric multigrid V(nu_pre, nu_post) cycles for the
// fixed-edge Poisson solve u = A u + g on one GPU (mxs/kernels/multigrid.hpp,
// docs/ARCHITECTURE.md "Multigrid").
//
// Per level it owns a u ping-pong pair and a g tile (TileGeom::aligned(w, h, 1,
// 1)); both fine u buffers carry the boundary ring, every coarser ring is 0 (a
// coarse level solves for an error). One stream. A V-cycle on level k:
//   1. nu_pre sweeps (one mg_smooth launch)      u_k[0] -> u_k[1]
//   2. g_{k+1} = 4 R (A u + g - u)               mg_residual_restrict
//   3. e_{k+1} = 0                               memset of u_{k+1}[0]
//   4. recurse; the coarsest level runs mg_coarse_solve
//   5. u_k[1] += P e_{k+1}                       mg_prolong_add
//   6. nu_post sweeps                            u_k[1] -> u_k[0]
// so the field is in u_0[0] between cycles. With cfg.graph the cycle is
// captured once as a linear hipGraph (one stream, no branches) and replayed;
// eager launches give the same bits.
#pragma once

#include <string>
#include <vector>

#include "mxs/kernels/kernels.hpp"
#include "mxs/runtime/hip_utils.hpp"
#include "mxs/runtime/tile_utils.hpp"

namespace mxs {

struct MultigridConfig {
  index_t width = 0, height = 0;
  double c_center = 0.2, c_neighbor = 0.2;
  int nu_pre = 2, nu_post = 2;
  double smoother_omega = 0.8;
  double coarse_reduction = 1e-3;
  bool graph = true;
};

struct MultigridResidual {
  double linf = 0.0, l2 = 0.0;
  index_t cells = 0;
};

struct MultigridSolve {
  bool converged = false;
  int cycles = 0;
  double residual = 0.0;
  std::string reason, norm;
  struct Check {
    int cycle;
    double linf, l2;
  };
  std::vector<Check> history;
};

// Cycles without a new best residual after which solve() stops ("stalled": the
// rounding floor of the element type).
constexpr int kMgStallCycles = 3;

template <typename T>
class MultigridSolver {
 public:
  using value_type = T;
  explicit MultigridSolver(const MultigridConfig& cfg);
  MultigridSolver(const MultigridSolver&) = delete;
  MultigridSolver& operator=(const MultigridSolver&) = delete;

  const MultigridConfig& config() const { return cfg_; }
  const std::vector<kernels::MgLevel>& levels() const { return plan_; }
  const TileGeom& geom() const { return lv_[0].geom; }

  // Boundary values of the fine ring: device pointers to width (top, bottom)
  // or height (left, right) values, nullptr leaves a side as it is. Written
  // into both fine buffers.
  void set_boundary(const T* top, const T* bottom, const T* left, const T* right);
  // g: a device tile of geom() whose core holds the source, or nullptr (g = 0).
  void set_source(const T* tile);
  // The field: device tiles of geom(); set_field takes the core only.
  void set_field(const T* tile);
  void field(T* tile);
  MultigridResidual residual();
  void vcycle(int n);
  MultigridSolve solve(double tol, int max_cycles, const std::string& norm);
  std::string graph_status() const { return graph_status_; }
  std::string note() const;
  int launches_per_cycle() const { return launches_; }

 private:
  struct Level {
    TileGeom geom;
    DeviceBuffer<T> u[2], g;
  };
  void enqueue_cycle();
  void enqueue_level(size_t k);
  bool capture();

  MultigridConfig cfg_;
  std::vector<kernels::MgLevel> plan_;
  std::vector<Level> lv_;
  kernels::MgSweepTable pre_, post_;
  kernels::MgCoarsePlan coarse_;
  Stream stream_;
  GraphExec graph_;
  bool graph_tried_ = false;
  std::string graph_status_ = "off";
  int launches_ = 0;
  ResidualReadback readback_;
};

}  // namespace mxs
