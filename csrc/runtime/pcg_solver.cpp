// PcgSolver<T> (mxs/runtime/pcg_solver.hpp).
#include "mxs/runtime/pcg_solver.hpp"

#include <algorithm>
#include <cmath>
#include <sstream>
#include <stdexcept>

namespace mxs {

template <typename T>
PcgSolver<T>::PcgSolver(const PcgConfig& cfg) : cfg_(cfg), sides_(kernels::ghost_sides_of(cfg.neumann)) {
  plan_ = kernels::pcg_plan_levels(cfg.width, cfg.height, cfg.c_center, cfg.c_neighbor, sides_);
  coarse_ = kernels::pcg_coarse_plan(plan_.back(), cfg.c_neighbor, cfg.coarse_reduction);
  geom_ = TileGeom::aligned(cfg.width, cfg.height, 1, 1, int(sizeof(T)));
  for (DeviceBuffer<T>* b : {&u_, &g_, &r_, &q_, &p_[0], &p_[1]}) {
    b->reset(geom_.alloc_elems());
    MXS_HIP_CHECK(hipMemsetAsync(b->get(), 0, b->bytes(), stream_.get()));
  }
  lv_.resize(plan_.size());
  for (size_t k = 0; k < plan_.size(); ++k) {
    Level& l = lv_[k];
    l.geom = TileGeom::aligned(plan_[k].width, plan_[k].height, 1, 1, int(sizeof(T)));
    l.smooth = kernels::mg_smoother_table(plan_[k].c0, cfg.c_neighbor, cfg.smoother_omega, cfg.nu);
    for (DeviceBuffer<T>* b : {&l.u[0], &l.u[1], &l.g}) {
      if (k == 0 && b == &l.g) continue;
      b->reset(l.geom.alloc_elems());
      MXS_HIP_CHECK(hipMemsetAsync(b->get(), 0, b->bytes(), stream_.get()));
    }
  }
  scalars_.reset(1);
  MXS_HIP_CHECK(hipMemsetAsync(scalars_.get(), 0, sizeof(kernels::PcgScalars), stream_.get()));
  residual_scalars_.reset(1);
  MXS_HIP_CHECK(hipMemsetAsync(residual_scalars_.get(), 0, sizeof(kernels::PcgScalars), stream_.get()));
  partials_.reset(2 * index_t(std::max(kernels::cg_grid_size(geom_), kernels::mgp_smooth_grid_size(geom_))));
  counter_.reset(1);
  MXS_HIP_CHECK(hipMemsetAsync(counter_.get(), 0, sizeof(unsigned), stream_.get()));
  residual_buf_.reset(2 + 2 * index_t(kernels::residual_grid_size(geom_)));
  residual_counter_.reset(1);
  residual_host_.reset(2);
  scalars_host_.reset(2);  // [0] the controls on their way up, [1] the readback
  // The coarse solve once, outside any capture (it raises its LDS limit on
  // first use); a source of 0 gives e = 0.
  Level& c = lv_.back();
  kernels::mgp_coarse_solve<T>(lv_.size() == 1 ? r_.get() : c.g.get(), c.u[0].get(), c.geom, coarse_.table, 1,
                               plan_.back().sides, nullptr, stream_.get());
  stream_.sync();
}

template <typename T>
void PcgSolver<T>::set_boundary(const T* top, const T* bottom, const T* left, const T* right) {
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
void PcgSolver<T>::set_source(const T* tile) {
  if (tile) MXS_HIP_CHECK(hipMemcpyAsync(g_.get(), tile, g_.bytes(), hipMemcpyDeviceToDevice, stream_.get()));
  else MXS_HIP_CHECK(hipMemsetAsync(g_.get(), 0, g_.bytes(), stream_.get()));
  stream_.sync();
}

template <typename T>
void PcgSolver<T>::set_field(const T* tile) {
  const TileGeom& g = geom_;
  const index_t off = g.core_offset();
  MXS_HIP_CHECK(hipMemcpy2DAsync(u_.get() + off, size_t(g.pitch) * sizeof(T), tile + off, size_t(g.pitch) * sizeof(T),
                                 size_t(g.width) * sizeof(T), size_t(g.height), hipMemcpyDeviceToDevice, stream_.get()));
  stream_.sync();
}

template <typename T>
void PcgSolver<T>::field(T* tile) {
  MXS_HIP_CHECK(hipMemcpyAsync(tile, u_.get(), u_.bytes(), hipMemcpyDeviceToDevice, stream_.get()));
  stream_.sync();
}

template <typename T>
CgResidual PcgSolver<T>::residual() {
  auto* norms = reinterpret_cast<kernels::ResidualNorms*>(residual_buf_.get());
  kernels::Stencil5Coeffs c{cfg_.c_center, cfg_.c_neighbor, false, -1.0};
  if (sides_.any_mirror()) {  // CgSolver::residual: pcg_start's residual into the scratch tile q
    kernels::pcg_start<T>(u_.get(), g_.get(), q_.get(), geom_, c, residual_scalars_.get(), partials_.get(),
                          counter_.get(), stream_.get(), sides_);
    MXS_HIP_CHECK(hipMemcpyAsync(scalars_host_.get() + 1, residual_scalars_.get(), sizeof(kernels::PcgScalars),
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
kernels::PcgScalars PcgSolver<T>::read_scalars() {
  MXS_HIP_CHECK(hipMemcpyAsync(scalars_host_.get() + 1, scalars_.get(), sizeof(kernels::PcgScalars),
                               hipMemcpyDeviceToHost, stream_.get()));
  stream_.spin_sync();
  return scalars_host_.get()[1];
}

template <typename T>
kernels::PcgScalars PcgSolver<T>::scalars() {
  return read_scalars();
}

template <typename T>
kernels::PcgScalars PcgSolver<T>::start(double tol, int max_iters, int norm) {
  hipStream_t s = stream_.get();
  kernels::PcgScalars& up = scalars_host_.get()[0];
  up = kernels::PcgScalars{};
  up.tol = tol;
  up.max_iters = max_iters;
  up.norm = norm;
  MXS_HIP_CHECK(hipMemcpyAsync(scalars_.get(), &up, sizeof(up), hipMemcpyHostToDevice, s));
  MXS_HIP_CHECK(hipMemsetAsync(counter_.get(), 0, sizeof(unsigned), s));
  // The first direction is fma(0, p_old, z): p_old has to be finite.
  MXS_HIP_CHECK(hipMemsetAsync(p_[0].get(), 0, p_[0].bytes(), s));
  const kernels::Stencil5Coeffs c{cfg_.c_center, cfg_.c_neighbor, false, -1.0};
  kernels::pcg_start<T>(u_.get(), g_.get(), r_.get(), geom_, c, scalars_.get(), partials_.get(), counter_.get(), s,
                        sides_);
  return read_scalars();
}

// z = M r into lv_[0].u[0]: level k's source is r (k == 0) or its own g, its
// iterate starts at 0 (mgp_smooth's start from zero), the pre-smooth writes
// u[1], the coarse correction is added there and the post-smooth writes u[0]. The last launch
// (the finest post-smooth, or the coarse solve of a single level) carries the
// dot epilogue.
template <typename T>
void PcgSolver<T>::enqueue_level(size_t k) {
  Level& l = lv_[k];
  const kernels::PcgLevel& pl = plan_[k];
  hipStream_t s = stream_.get();
  const T* src = k == 0 ? r_.get() : l.g.get();
  kernels::PcgScalars* dot = k == 0 ? scalars_.get() : nullptr;
  if (k + 1 == lv_.size()) {
    kernels::mgp_coarse_solve<T>(src, l.u[0].get(), l.geom, coarse_.table, coarse_.repeats, pl.sides, dot, s);
    ++launches_;
    return;
  }
  Level& c = lv_[k + 1];
  const kernels::Stencil5Coeffs co{pl.c0, cfg_.c_neighbor, false, -1.0};
  // Every level starts from e = 0: the pre-smooth takes it as given, no tile is zeroed or read.
  kernels::mgp_smooth<T>(static_cast<const T*>(nullptr), l.u[1].get(), src, l.geom, l.smooth, pl.sides, nullptr, nullptr,
                         nullptr, s);
  kernels::mgp_residual_restrict<T>(l.u[1].get(), src, l.geom, pl.sides, c.g.get(), c.geom, co, s);
  launches_ += 2;
  enqueue_level(k + 1);
  kernels::mgp_prolong_add<T>(c.u[0].get(), c.geom, l.u[1].get(), l.geom, s, pl.sides);
  kernels::mgp_smooth<T>(l.u[1].get(), l.u[0].get(), src, l.geom, l.smooth, pl.sides, dot,
                         dot ? partials_.get() : nullptr, dot ? counter_.get() : nullptr, s);
  launches_ += 2;
}

// Iterations j = parity, parity + 1, ...: j reads p[j % 2] and writes p[(j + 1) % 2].
template <typename T>
void PcgSolver<T>::enqueue_iterations(int n, int parity) {
  hipStream_t s = stream_.get();
  const kernels::Stencil5Coeffs c{cfg_.c_center, cfg_.c_neighbor, false, -1.0};
  T* z = lv_[0].u[0].get();
  for (int i = 0; i < n; ++i) {
    const int a = (parity + i) & 1;
    launches_ = 0;
    enqueue_level(0);
    kernels::pcg_apply<T>(z, p_[a].get(), p_[a ^ 1].get(), q_.get(), geom_, c, scalars_.get(), partials_.get(),
                          counter_.get(), s, sides_);
    kernels::pcg_update<T>(u_.get(), r_.get(), p_[a ^ 1].get(), q_.get(), geom_, scalars_.get(), partials_.get(),
                           counter_.get(), s);
    launches_ += 2;
  }
}

template <typename T>
bool PcgSolver<T>::capture(int iters) {
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
CgSolve PcgSolver<T>::solve(double tol, int max_iters, const std::string& norm, int check_every) {
  if (norm != "linf" && norm != "l2")
    throw std::invalid_argument("preconditioned CG: norm must be 'linf' or 'l2', got '" + norm + "'");
  if (!(tol >= 0.0) || max_iters < 0 || check_every < 1)
    throw std::invalid_argument("preconditioned CG: solve needs tol >= 0, max_iters >= 0 and check_every >= 1");
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
  for (;;) {  // one run from pcg_start
    kernels::PcgScalars sc = start(tol, remaining, norm_id);
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
std::string PcgSolver<T>::note() const {
  std::ostringstream os;
  os << "multigrid-preconditioned CG " << cfg_.width << "x" << cfg_.height << ", c_center " << cfg_.c_center
     << ", c_neighbor " << cfg_.c_neighbor
     << (sides_.any_mirror() ? ", Neumann sides " + kernels::ghost_sides_names(sides_) : std::string()) << ", V(" << cfg_.nu << "," << cfg_.nu << ") over " << plan_.size()
     << " levels down to " << plan_.back().width << "x" << plan_.back().height << ", smoother omega "
     << cfg_.smoother_omega << ", coarse solve " << coarse_.repeats << " x " << coarse_.table.n
     << " Chebyshev sweeps (rho " << coarse_.rho << "), graph " << graph_status_;
  if (graph_.valid()) os << " (" << graph_iters_ << " iterations per launch)";
  return os.str();
}

template class PcgSolver<float>;
template class PcgSolver<double>;

}  // namespace mxs
