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
// A reported convergence is confirmed on the true residual, else a restart:
// the host protocol is cg_drive's (mxs/runtime/cg_protocol.hpp).
//
// CgSolverBase<T, Scalars> holds what CgSolver and PcgSolver share: the tiles,
// the scalar blocks, the stream and the graph, the setters and getters, the
// capture and solve(), which runs cg_drive (mxs/runtime/cg_protocol.hpp). A
// solver supplies its start launch, its iterations and its note. step() is
// solve() for one implicit heat step (mxs/kernels/heat.hpp): its first start
// launch is the fused heat start, which also makes the right-hand side g.
//
// cfg.neumann names the Neumann sides (mxs/kernels/cg.hpp "GhostSides"): the
// kernels then read the ghost of such a side as edge + ring (cg_start) or as
// the edge cell of the direction itself (cg_apply), and the true residual is
// that of the same operator. With none the launches are those of before.
#pragma once

#include <string>
#include <vector>

#include "mxs/kernels/kernels.hpp"
#include "mxs/runtime/cg_protocol.hpp"
#include "mxs/runtime/hip_utils.hpp"
#include "mxs/runtime/tile_utils.hpp"

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

// Scalars: the device scalar block, kernels::CgScalars or kernels::PcgScalars.
template <typename T, typename Scalars>
class CgSolverBase {
 public:
  using value_type = T;
  CgSolverBase(const CgSolverBase&) = delete;
  CgSolverBase& operator=(const CgSolverBase&) = delete;
  virtual ~CgSolverBase() = default;

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
  // With a Neumann side it is the start kernel's residual (the ghost is edge +
  // ring), taken into scratch tiles (q; plain CG also p[1]) and a scalar block
  // of its own; a solve in progress must not call it.
  CgResidual residual();
  CgSolve solve(double tol, int max_iters, const std::string& norm, int check_every);
  // One implicit heat step u -> u' (mxs/kernels/heat.hpp): solve() with one
  // difference, the first run's start launch is the fused kernel (cg_heat_start
  // / pcg_heat_start), which makes the step's right-hand side from u as it
  // stands (and the step source) and writes it into g: every step overwrites
  // g, so set_source() is not the way to give a step its source. Restart runs,
  // residual() and the confirmation on the true residual use the ordinary start
  // on the stored g, so after a step residual() is that step's true residual.
  // Throws unless the solver's (c_center, c_neighbor) are exactly (0, hc.c1).
  CgSolve step(const kernels::HeatCoeffs& hc, double tol, int max_iters, const std::string& norm, int check_every);
  // q = dt f of the steps to come: a device tile of geom() whose core holds it
  // (copied into a tile of the solver's own, allocated on first use), or nullptr
  // for none: the steps then run the no-source kernel. It is not g.
  void set_step_source(const T* tile);
  // The device scalar block as it stands (a synchronising read).
  Scalars scalars() { return read_scalars(); }
  std::string graph_status() const { return graph_status_; }
  virtual std::string note() const = 0;

 protected:
  // who: the prefix of solve()'s argument errors.
  CgSolverBase(const char* who, double c_center, double c_neighbor, bool graph, const kernels::GhostSides& sides)
      : who_(who), c_center_(c_center), c_neighbor_(c_neighbor), graph_on_(graph), sides_(sides) {}
  // The shared buffers, zeroed on stream_ (not synchronised); partials_ is the solver's to size.
  void allocate(index_t width, index_t height);
  kernels::Stencil5Coeffs coeffs() const { return {c_center_, c_neighbor_, false, -1.0}; }

  // The start kernel into (r, p[0], scalars_) with whatever the solver puts
  // before it, or, into_scratch, its residual alone into q and residual_scalars_.
  virtual void launch_start(bool into_scratch) = 0;
  // The fused start of a heat step into (g, r, p[0], scalars_); q: the step source or nullptr.
  virtual void launch_heat_start(const kernels::HeatCoeffs& hc, const T* q) = 0;
  // Iterations j = parity, parity + 1, ...: j reads p[j % 2] and writes p[(j + 1) % 2].
  virtual void enqueue_iterations(int n, int parity) = 0;

  const char* who_;
  double c_center_, c_neighbor_;
  bool graph_on_;
  kernels::GhostSides sides_;
  TileGeom geom_;
  DeviceBuffer<T> u_, g_, r_, q_, p_[2];
  DeviceBuffer<T> step_q_;  // the step source, allocated by the first set_step_source(tile)
  bool step_source_ = false;
  DeviceBuffer<Scalars> scalars_, residual_scalars_;
  DeviceBuffer<double> partials_;
  DeviceBuffer<unsigned> counter_;
  ResidualReadback readback_;
  PinnedBuffer<Scalars> scalars_host_;  // [0] the controls on their way up, [1] the readback
  Stream stream_;
  GraphExec graph_;
  int graph_iters_ = 0;
  std::string graph_status_ = "off";

 private:
  bool capture(int iters);
  // heat: the run starts with the fused heat start instead of launch_start(false).
  Scalars start(double tol, int max_iters, int norm, const kernels::HeatCoeffs* heat);
  CgSolve drive(const kernels::HeatCoeffs* heat, double tol, int max_iters, const std::string& norm, int check_every);
  Scalars read_scalars();
};

template <typename T>
class CgSolver : public CgSolverBase<T, kernels::CgScalars> {
 public:
  explicit CgSolver(const CgConfig& cfg);
  const CgConfig& config() const { return cfg_; }
  std::string note() const override;

 private:
  void launch_start(bool into_scratch) override;
  void launch_heat_start(const kernels::HeatCoeffs& hc, const T* q) override;
  void enqueue_iterations(int n, int parity) override;

  CgConfig cfg_;
};

}  // namespace mxs
