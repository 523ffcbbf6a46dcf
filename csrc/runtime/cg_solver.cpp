// CgSolverBase<T, Scalars> and CgSolver<T> (mxs/runtime/cg_solver.hpp).
#include "mxs/runtime/cg_solver.hpp"

#include <cmath>
#include <sstream>
#include <stdexcept>

namespace mxs {

template <typename T, typename S>
void CgSolverBase<T, S>::allocate(index_t width, index_t height) {
  geom_ = TileGeom::aligned(width, height, 1, 1, int(sizeof(T)));
  for (DeviceBuffer<T>* b : {&u_, &g_, &r_, &q_, &p_[0], &p_[1]}) {
    b->reset(geom_.alloc_elems());
    MXS_HIP_CHECK(hipMemsetAsync(b->get(), 0, b->bytes(), stream_.get()));
  }
  for (DeviceBuffer<S>* b : {&scalars_, &residual_scalars_}) {
    b->reset(1);
    MXS_HIP_CHECK(hipMemsetAsync(b->get(), 0, sizeof(S), stream_.get()));
  }
  counter_.reset(1);
  MXS_HIP_CHECK(hipMemsetAsync(counter_.get(), 0, sizeof(unsigned), stream_.get()));
  readback_.reset(geom_);
  scalars_host_.reset(2);
}

template <typename T, typename S>
void CgSolverBase<T, S>::set_boundary(const T* top, const T* bottom, const T* left, const T* right) {
  copy_ring_sides(u_.get(), geom_, top, bottom, left, right, stream_.get());
  stream_.sync();
}

template <typename T, typename S>
void CgSolverBase<T, S>::set_source(const T* tile) {
  if (tile) MXS_HIP_CHECK(hipMemcpyAsync(g_.get(), tile, g_.bytes(), hipMemcpyDeviceToDevice, stream_.get()));
  else MXS_HIP_CHECK(hipMemsetAsync(g_.get(), 0, g_.bytes(), stream_.get()));
  stream_.sync();
}

template <typename T, typename S>
void CgSolverBase<T, S>::set_field(const T* tile) {
  const TileGeom& g = geom_;
  const index_t off = g.core_offset();
  MXS_HIP_CHECK(hipMemcpy2DAsync(u_.get() + off, size_t(g.pitch) * sizeof(T), tile + off, size_t(g.pitch) * sizeof(T),
                                 size_t(g.width) * sizeof(T), size_t(g.height), hipMemcpyDeviceToDevice, stream_.get()));
  stream_.sync();
}

template <typename T, typename S>
void CgSolverBase<T, S>::field(T* tile) {
  MXS_HIP_CHECK(hipMemcpyAsync(tile, u_.get(), u_.bytes(), hipMemcpyDeviceToDevice, stream_.get()));
  stream_.sync();
}

template <typename T, typename S>
CgResidual CgSolverBase<T, S>::residual() {
  if (!sides_.any_mirror())
    return readback_.template read<CgResidual>(u_.get(), g_.get(), geom_, c_center_, c_neighbor_, stream_);
  // stencil5_residual knows only the ring: the start kernel computes exactly this residual
  launch_start(true);
  MXS_HIP_CHECK(hipMemcpyAsync(scalars_host_.get() + 1, residual_scalars_.get(), sizeof(S), hipMemcpyDeviceToHost,
                               stream_.get()));
  stream_.spin_sync();
  CgResidual r;
  r.linf = scalars_host_.get()[1].linf;
  r.l2 = std::sqrt(scalars_host_.get()[1].rr);
  r.cells = geom_.width * geom_.height;
  return r;
}

template <typename T, typename S>
S CgSolverBase<T, S>::read_scalars() {
  MXS_HIP_CHECK(hipMemcpyAsync(scalars_host_.get() + 1, scalars_.get(), sizeof(S), hipMemcpyDeviceToHost, stream_.get()));
  stream_.spin_sync();
  return scalars_host_.get()[1];
}

template <typename T, typename S>
S CgSolverBase<T, S>::start(double tol, int max_iters, int norm, const kernels::HeatCoeffs* heat) {
  hipStream_t s = stream_.get();
  S& up = scalars_host_.get()[0];
  up = S{};
  up.tol = tol;
  up.max_iters = max_iters;
  up.norm = norm;
  MXS_HIP_CHECK(hipMemcpyAsync(scalars_.get(), &up, sizeof(up), hipMemcpyHostToDevice, s));
  MXS_HIP_CHECK(hipMemsetAsync(counter_.get(), 0, sizeof(unsigned), s));
  if (heat) launch_heat_start(*heat, step_source_ ? step_q_.get() : nullptr);
  else launch_start(false);
  return read_scalars();
}

template <typename T, typename S>
bool CgSolverBase<T, S>::capture(int iters) {
  graph_.reset();
  graph_iters_ = iters;
  return capture_linear(stream_, graph_, graph_status_, [&] { enqueue_iterations(iters, 0); });
}

template <typename T, typename S>
void CgSolverBase<T, S>::set_step_source(const T* tile) {
  step_source_ = tile != nullptr;
  if (!tile) return;
  if (step_q_.size() == 0) step_q_.reset(geom_.alloc_elems());
  MXS_HIP_CHECK(hipMemcpyAsync(step_q_.get(), tile, step_q_.bytes(), hipMemcpyDeviceToDevice, stream_.get()));
  stream_.sync();
}

template <typename T, typename S>
CgSolve CgSolverBase<T, S>::solve(double tol, int max_iters, const std::string& norm, int check_every) {
  return drive(nullptr, tol, max_iters, norm, check_every);
}

template <typename T, typename S>
CgSolve CgSolverBase<T, S>::step(const kernels::HeatCoeffs& hc, double tol, int max_iters, const std::string& norm,
                                 int check_every) {
  if (c_center_ != 0.0 || c_neighbor_ != hc.c1) {
    std::ostringstream os;
    os.precision(17);
    os << who_ << ": step() needs a solver built with the step's own weights (c_center, c_neighbor) = (0, " << hc.c1
       << "); this one has (" << c_center_ << ", " << c_neighbor_ << ")";
    throw std::invalid_argument(os.str());
  }
  return drive(&hc, tol, max_iters, norm, check_every);
}

// heat: the first run starts with the fused heat start; a restart takes the ordinary one on the stored g.
template <typename T, typename S>
CgSolve CgSolverBase<T, S>::drive(const kernels::HeatCoeffs* heat, double tol, int max_iters, const std::string& norm,
                                  int check_every) {
  int block = check_every;
  if (graph_on_) block += block & 1;  // even: the p ping-pong closes inside the graph
  int parity = 0;                     // of the eager path: the p buffer the next block reads
  const auto progress = [](const S& sc) { return CgProgress{sc.status, sc.iteration, sc.rr, sc.linf}; };
  return cg_drive(
      who_, tol, max_iters, norm, check_every,
      [&](double run_tol, int remaining, int norm_id) {
        // Here, not above: cg_drive has checked the arguments by now.
        if (graph_on_ && graph_iters_ != block) capture(block);
        parity = 0;
        const kernels::HeatCoeffs* first = heat;
        heat = nullptr;
        return progress(start(run_tol, remaining, norm_id, first));
      },
      [&] {
        if (graph_.valid()) {
          graph_.launch(stream_.get());
        } else {
          enqueue_iterations(block, parity);
          parity = (parity + block) & 1;
        }
        return progress(read_scalars());
      },
      [&] { return residual(); });
}

template class CgSolverBase<float, kernels::CgScalars>;
template class CgSolverBase<double, kernels::CgScalars>;
template class CgSolverBase<float, kernels::PcgScalars>;
template class CgSolverBase<double, kernels::PcgScalars>;

// ------------------------------------------------------------------ CgSolver
template <typename T>
CgSolver<T>::CgSolver(const CgConfig& cfg)
    : CgSolverBase<T, kernels::CgScalars>("conjugate gradients", cfg.c_center, cfg.c_neighbor, cfg.graph,
                                          kernels::ghost_sides_of(cfg.neumann)),
      cfg_(cfg) {
  kernels::cg_check_sides(cfg.c_center, cfg.c_neighbor, this->sides_);
  if (cfg.width < 1 || cfg.height < 1) throw std::invalid_argument("conjugate gradients: the grid must be non-empty");
  this->allocate(cfg.width, cfg.height);
  this->partials_.reset(2 * index_t(kernels::cg_grid_size(this->geom_)));
  this->stream_.sync();
}

template <typename T>
void CgSolver<T>::launch_start(bool into_scratch) {
  // The scratch run stores its first direction too: into p[1], which no solve in progress owns.
  kernels::cg_start<T>(this->u_.get(), this->g_.get(), (into_scratch ? this->q_ : this->r_).get(),
                       this->p_[into_scratch ? 1 : 0].get(), this->geom_, this->coeffs(),
                       (into_scratch ? this->residual_scalars_ : this->scalars_).get(), this->partials_.get(),
                       this->counter_.get(), this->stream_.get(), this->sides_);
}

template <typename T>
void CgSolver<T>::launch_heat_start(const kernels::HeatCoeffs& hc, const T* q) {
  kernels::cg_heat_start<T>(this->u_.get(), q, this->g_.get(), this->r_.get(), this->p_[0].get(), this->geom_, hc,
                            this->scalars_.get(), this->partials_.get(), this->counter_.get(), this->stream_.get(),
                            this->sides_);
}

template <typename T>
void CgSolver<T>::enqueue_iterations(int n, int parity) {
  hipStream_t s = this->stream_.get();
  const kernels::Stencil5Coeffs c = this->coeffs();
  auto& p = this->p_;
  for (int i = 0; i < n; ++i) {
    const int a = (parity + i) & 1;
    kernels::cg_apply<T>(this->r_.get(), p[a].get(), p[a ^ 1].get(), this->q_.get(), this->geom_, c,
                         this->scalars_.get(), this->partials_.get(), this->counter_.get(), s, this->sides_);
    kernels::cg_update<T>(this->u_.get(), this->r_.get(), p[a ^ 1].get(), this->q_.get(), this->geom_,
                          this->scalars_.get(), this->partials_.get(), this->counter_.get(), s);
  }
}

template <typename T>
std::string CgSolver<T>::note() const {
  std::ostringstream os;
  os << "conjugate gradients " << cfg_.width << "x" << cfg_.height << ", c_center " << cfg_.c_center << ", c_neighbor "
     << cfg_.c_neighbor
     << (this->sides_.any_mirror() ? ", Neumann sides " + kernels::ghost_sides_names(this->sides_) : std::string())
     << ", 2 kernels per iteration (cg_apply, cg_update) on " << kernels::cg_grid_size(this->geom_)
     << " workgroups at most, graph " << this->graph_status_;
  if (this->graph_.valid()) os << " (" << this->graph_iters_ << " iterations per launch)";
  return os.str();
}

template class CgSolver<float>;
template class CgSolver<double>;

}  // namespace mxs
