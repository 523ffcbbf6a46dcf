// CgSolver<T>: conjugate gradients for the fixed-edge solve u = A u + g on one
// GPU, any W x H >= 1 and any admissible weights (mxs/kernels/cg.hpp,
// docs/ARCHITECTURE.md "Conjugate gradients").
//
// It owns the tiles u, g, r, q and a p ping-pong pair of TileGeom::aligned(w, h,
// 1, 1), the device scalar block and one stream. solve() enqueues cg_start,
// then blocks of iterations (cg_apply + cg_update each), then a pinned read of
// the scalar block. The device decides when the iteration stops (a launch
// whose status is not 0 at entry stores nothing), so the host's cadence cannot
// change a bit of the result. With cfg.graph a block is one linear captured
// hipGraph (one stream, no branches, an even number of iterations so the p
// ping-pong closes); eager launches give the same bits.
//
// The device's test is on the recursive residual. When it reports convergence
// the host takes the true residual (stencil5_residual with the source); if
// that is above tol the solve restarts from cg_start with the iterations
// already spent counted, and after kCgMaxRestarts restarts it ends "stalled"
// (the element type's floor).
//
// cfg.neumann names the Neumann sides (mxs/kernels/cg.hpp "GhostSides"): the
// kernels then read the ghost of such a side as edge + ring (cg_start) or as
// the edge cell of the direction itself (cg_apply), and the true residual is
// that of the same operator. With none the launches are those of before.
#pragma once

#include <string>
#include <vector>

#include "mxs/kernels/kernels.hpp"
#include "mxs/runtime/hip_utils.hpp"

namespace mxs {

struct CgConfig {
  index_t width = 0, height = 0;
  double c_center = 0.2, c_neighbor = 0.2;
  bool graph = true;
  // The Neumann sides by name (top, bottom, left, right); every other side is
  // Dirichlet. On a Neumann side the ring holds the prescribed outward
  // difference d = u_ghost - u_edge (0: insulated) and the ghost reads edge + d.
  std::vector<std::string> neumann;
};

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

template <typename T>
class CgSolver {
 public:
  using value_type = T;
  explicit CgSolver(const CgConfig& cfg);
  CgSolver(const CgSolver&) = delete;
  CgSolver& operator=(const CgSolver&) = delete;

  const CgConfig& config() const { return cfg_; }
  const TileGeom& geom() const { return geom_; }

  // Boundary values of the ring: device pointers to width (top, bottom) or
  // height (left, right) values, nullptr leaves a side as it is.
  void set_boundary(const T* top, const T* bottom, const T* left, const T* right);
  // g: a device tile of geom() whose core holds the source, or nullptr (g = 0).
  void set_source(const T* tile);
  // The field: device tiles of geom(); set_field takes the core only.
  void set_field(const T* tile);
  void field(T* tile);
  // Norms of the true residual (A u + g) - u: stencil5_residual with the source.
  // With a Neumann side it is cg_start's residual (the ghost is edge + ring),
  // taken into the scratch tiles q and p[1] and a scalar block of its own; a
  // solve in progress must not call it.
  CgResidual residual();
  CgSolve solve(double tol, int max_iters, const std::string& norm, int check_every);
  // The device scalar block as it stands (a synchronising read).
  kernels::CgScalars scalars();
  std::string graph_status() const { return graph_status_; }
  std::string note() const;

 private:
  void enqueue_iterations(int n, int parity);
  bool capture(int iters);
  kernels::CgScalars start(double tol, int max_iters, int norm);
  kernels::CgScalars read_scalars();

  CgConfig cfg_;
  kernels::GhostSides sides_;
  TileGeom geom_;
  DeviceBuffer<T> u_, g_, r_, q_, p_[2];
  DeviceBuffer<kernels::CgScalars> scalars_, residual_scalars_;
  DeviceBuffer<double> partials_, residual_buf_;
  DeviceBuffer<unsigned> counter_, residual_counter_;
  PinnedBuffer<kernels::CgScalars> scalars_host_;
  PinnedBuffer<double> residual_host_;
  Stream stream_;
  GraphExec graph_;
  int graph_iters_ = 0;
  std::string graph_status_ = "off";
};

}  // namespace mxs
