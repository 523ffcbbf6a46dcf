// CgSolver<T> (mxs/runtime/cg_solver.hpp).
#include "mxs/runtime/cg_solver.hpp"

#include <cmath>
#include <sstream>
#include <stdexcept>

namespace mxs {

template <typename T>
CgSolver<T>::CgSolver(const CgConfig& cfg) : cfg_(cfg), sides_(kernels::ghost_sides_of(cfg.neumann)) {
  kernels::cg_check_sides(cfg.c_center, cfg.c_neighbor, sides_);
  if (cfg.width < 1 || cfg.height < 1) throw std::invalid_argument("conjugate gradients: the grid must be non-empty");
  geom_ = TileGeom::aligned(cfg.width, cfg.height, 1, 1, int(sizeof(T)));
  for (DeviceBuffer<T>* b : {&u_, &g_, &r_, &q_, &p_[0], &p_[1]}) {
    b->reset(geom_.alloc_elems());
    MXS_HIP_CHECK(hipMemsetAsync(b->get(), 0, b->bytes(), stream_.get()));
  }
  scalars_.reset(1);
  MXS_HIP_CHECK(hipMemsetAsync(scalars_.get(), 0, sizeof(kernels::CgScalars), stream_.get()));
  residual_scalars_.reset(1);
  MXS_HIP_CHECK(hipMemsetAsync(residual_scalars_.get(), 0, sizeof(kernels::CgScalars), stream_.get()));
  partials_.reset(2 * index_t(kernels::cg_grid_size(geom_)));
  counter_.reset(1);
  MXS_HIP_CHECK(hipMemsetAsync(counter_.get(), 0, sizeof(unsigned), stream_.get()));
  residual_buf_.reset(2 + 2 * index_t(kernels::residual_grid_size(geom_)));
  residual_counter_.reset(1);
  residual_host_.reset(2);
  scalars_host_.reset(2);  // [0] the controls on their way up, [1] the readback
  stream_.sync();
}

template <typename T>
void CgSolver<T>::set_boundary(const T* top, const T* bottom, const T* left, const T* right) {
  const TileGeom& g = geom_;
  const index_t off = g.core_offset();
  T* u = u_.get();
  hipStream_t s = stream_.get();
  if (top) MXS_HIP_CHECK(hipMemcpyAsync(u + off - g.pitch, top, size_t(g.width) * sizeof(T), hipMemcpyDeviceToDevice, s));
  if (bottom)
    MXS_HIP_CHECK(hipMemcpyAsync(u + off + g.height * g.pitch, bottom, size_t(g.width) * sizeof(T),
                                 hipMemcpyDeviceToDevice, s));
  if (left)
    MXS_HIP_CHECK(hipMemcpy2DAsync(u + off - 1, size_t(g.pitch) * sizeof(T), left, sizeof(T), sizeof(T), size_t(g.height),
                                   hipMemcpyDeviceToDevice, s));
  if (right)
    MXS_HIP_CHECK(hipMemcpy2DAsync(u + off + g.width, size_t(g.pitch) * sizeof(T), right, sizeof(T), sizeof(T),
                                   size_t(g.height), hipMemcpyDeviceToDevice, s));
  stream_.sync();
}

template <typename T>
void CgSolver<T>::set_source(const T* tile) {
  if (tile) MXS_HIP_CHECK(hipMemcpyAsync(g_.get(), tile, g_.bytes(), hipMemcpyDeviceToDevice, stream_.get()));
  else MXS_HIP_CHECK(hipMemsetAsync(g_.get(), 0, g_.bytes(), stream_.get()));
  stream_.sync();
}

template <typename T>
void CgSolver<T>::set_field(const T* tile) {
  const TileGeom& g = geom_;
  const index_t off = g.core_offset();
  MXS_HIP_CHECK(hipMemcpy2DAsync(u_.get() + off, size_t(g.pitch) * sizeof(T), tile + off, size_t(g.pitch) * sizeof(T),
                                 size_t(g.width) * sizeof(T), size_t(g.height), hipMemcpyDeviceToDevice, stream_.get()));
  stream_.sync();
}

template <typename T>
void CgSolver<T>::field(T* tile) {
  MXS_HIP_CHECK(hipMemcpyAsync(tile, u_.get(), u_.bytes(), hipMemcpyDeviceToDevice, stream_.get()));
  stream_.sync();
}

template <typename T>
CgResidual CgSolver<T>::residual() {
  auto* norms = reinterpret_cast<kernels::ResidualNorms*>(residual_buf_.get());
  kernels::Stencil5Coeffs c{cfg_.c_center, cfg_.c_neighbor, false, -1.0};
  if (sides_.any_mirror()) {  // stencil5_residual knows only the ring: cg_start computes exactly this residual
    kernels::cg_start<T>(u_.get(), g_.get(), q_.get(), p_[1].get(), geom_, c, residual_scalars_.get(), partials_.get(),
                         counter_.get(), stream_.get(), sides_);
    MXS_HIP_CHECK(hipMemcpyAsync(scalars_host_.get() + 1, residual_scalars_.get(), sizeof(kernels::CgScalars),
                                 hipMemcpyDeviceToHost, stream_.get()));
    stream_.spin_sync();
    CgResidual r;
    r.linf = scalars_host_.get()[1].linf;
    r.l2 = std::sqrt(scalars_host_.get()[1].rr);
    r.cells = geom_.width * geom_.height;
    return r;
  }
  kernels::stencil5_residual<T>(u_.get(), geom_, c, norms, residual_buf_.get() + 2, residual_counter_.get(),
                                stream_.get(), g_.get());
  MXS_HIP_CHECK(hipMemcpyAsync(residual_host_.get(), norms, sizeof(kernels::ResidualNorms), hipMemcpyDeviceToHost,
                               stream_.get()));
  stream_.spin_sync();
  CgResidual r;
  r.linf = residual_host_.get()[0];
  r.l2 = std::sqrt(residual_host_.get()[1]);
  r.cells = geom_.width * geom_.height;
  return r;
}

template <typename T>
kernels::CgScalars CgSolver<T>::read_scalars() {
  MXS_HIP_CHECK(hipMemcpyAsync(scalars_host_.get() + 1, scalars_.get(), sizeof(kernels::CgScalars), hipMemcpyDeviceToHost,
                               stream_.get()));
  stream_.spin_sync();
  return scalars_host_.get()[1];
}

template <typename T>
kernels::CgScalars CgSolver<T>::scalars() {
  return read_scalars();
}

template <typename T>
kernels::CgScalars CgSolver<T>::start(double tol, int max_iters, int norm) {
  hipStream_t s = stream_.get();
  kernels::CgScalars& up = scalars_host_.get()[0];
  up = kernels::CgScalars{};
  up.tol = tol;
  up.max_iters = max_iters;
  up.norm = norm;
  MXS_HIP_CHECK(hipMemcpyAsync(scalars_.get(), &up, sizeof(up), hipMemcpyHostToDevice, s));
  MXS_HIP_CHECK(hipMemsetAsync(counter_.get(), 0, sizeof(unsigned), s));
  const kernels::Stencil5Coeffs c{cfg_.c_center, cfg_.c_neighbor, false, -1.0};
  kernels::cg_start<T>(u_.get(), g_.get(), r_.get(), p_[0].get(), geom_, c, scalars_.get(), partials_.get(),
                       counter_.get(), s, sides_);
  return read_scalars();
}

// Iterations j = parity, parity + 1, ...: j reads p[j % 2] and writes p[(j + 1) % 2].
template <typename T>
void CgSolver<T>::enqueue_iterations(int n, int parity) {
  hipStream_t s = stream_.get();
  const kernels::Stencil5Coeffs c{cfg_.c_center, cfg_.c_neighbor, false, -1.0};
  for (int i = 0; i < n; ++i) {
    const int a = (parity + i) & 1;
    kernels::cg_apply<T>(r_.get(), p_[a].get(), p_[a ^ 1].get(), q_.get(), geom_, c, scalars_.get(), partials_.get(),
                         counter_.get(), s, sides_);
    kernels::cg_update<T>(u_.get(), r_.get(), p_[a ^ 1].get(), q_.get(), geom_, scalars_.get(), partials_.get(),
                          counter_.get(), s);
  }
}

template <typename T>
bool CgSolver<T>::capture(int iters) {
  graph_.reset();
  graph_iters_ = iters;
  hipGraph_t g = nullptr;
  if (hipStreamBeginCapture(stream_.get(), hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    graph_status_ = "hipStreamBeginCapture failed";
    return false;
  }
  bool ok = true;
  try {
    enqueue_iterations(iters, 0);
  } catch (const std::exception& e) {
    graph_status_ = std::string("capture failed: ") + e.what();
    ok = false;
  }
  const hipError_t end = hipStreamEndCapture(stream_.get(), &g);
  if (!ok || end != hipSuccess || g == nullptr) {
    (void)hipGetLastError();
    if (ok) graph_status_ = "hipStreamEndCapture failed";
    if (g) (void)hipGraphDestroy(g);
    return false;
  }
  if (!graph_.adopt(g)) {
    graph_status_ = "hipGraphInstantiate failed";
    return false;
  }
  graph_.upload(stream_.get());
  graph_status_ = "captured";
  return true;
}

template <typename T>
CgSolve CgSolver<T>::solve(double tol, int max_iters, const std::string& norm, int check_every) {
  if (norm != "linf" && norm != "l2")
    throw std::invalid_argument("conjugate gradients: norm must be 'linf' or 'l2', got '" + norm + "'");
  if (!(tol >= 0.0) || max_iters < 0 || check_every < 1)
    throw std::invalid_argument("conjugate gradients: solve needs tol >= 0, max_iters >= 0 and check_every >= 1");
  const int norm_id = norm == "linf" ? kernels::kCgNormLinf : kernels::kCgNormL2;
  int block = check_every;
  if (cfg_.graph) {
    block += block & 1;  // even: the p ping-pong closes inside the graph
    if (graph_iters_ != block) capture(block);
  }
  CgSolve out;
  out.norm = norm;
  int remaining = max_iters;
  bool have_true = false;
  for (;;) {  // one run from cg_start
    kernels::CgScalars sc = start(tol, remaining, norm_id);
    out.history.push_back({out.iterations, sc.linf, std::sqrt(sc.rr)});
    int parity = 0;
    while (sc.status == kernels::kCgRunning) {
      if (graph_.valid()) {
        graph_.launch(stream_.get());
      } else {
        enqueue_iterations(block, parity);
        parity = (parity + block) & 1;
      }
      sc = read_scalars();
      out.history.push_back({out.iterations + sc.iteration, sc.linf, std::sqrt(sc.rr)});
    }
    out.iterations += sc.iteration;
    remaining -= sc.iteration;
    if (sc.status == kernels::kCgConverged) {
      const CgResidual t = residual();
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
    const CgResidual t = residual();
    out.residual = norm_id == kernels::kCgNormLinf ? t.linf : t.l2;
  }
  return out;
}

template <typename T>
std::string CgSolver<T>::note() const {
  std::ostringstream os;
  os << "conjugate gradients " << cfg_.width << "x" << cfg_.height << ", c_center " << cfg_.c_center << ", c_neighbor "
     << cfg_.c_neighbor << (sides_.any_mirror() ? ", Neumann sides " + kernels::ghost_sides_names(sides_) : std::string())
     << ", 2 kernels per iteration (cg_apply, cg_update) on " << kernels::cg_grid_size(geom_)
     << " workgroups at most, graph " << graph_status_;
  if (graph_.valid()) os << " (" << graph_iters_ << " iterations per launch)";
  return os.str();
}

template class CgSolver<float>;
template class CgSolver<double>;

}  // namespace mxs
