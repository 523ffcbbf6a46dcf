// MultigridSolver<T> (mxs/runtime/multigrid_solver.hpp).
#include "mxs/runtime/multigrid_solver.hpp"

#include <cmath>
#include <sstream>
#include <stdexcept>

namespace mxs {

template <typename T>
MultigridSolver<T>::MultigridSolver(const MultigridConfig& cfg) : cfg_(cfg) {
  kernels::mg_check_operator(cfg.c_center, cfg.c_neighbor);
  plan_ = kernels::mg_plan_levels(cfg.width, cfg.height);
  if (plan_.size() < 2)
    throw std::invalid_argument("multigrid: " + std::to_string(cfg.width) + " x " + std::to_string(cfg.height) +
                                " has a single level (it coarsens only while both sides are odd, >= 3 and the larger "
                                "is above " + std::to_string(kernels::kMgCoarsenAbove) +
                                "): nothing to cycle over, use the relaxation solver");
  pre_ = kernels::mg_smoother_table(cfg.c_center, cfg.c_neighbor, cfg.smoother_omega, cfg.nu_pre);
  post_ = kernels::mg_smoother_table(cfg.c_center, cfg.c_neighbor, cfg.smoother_omega, cfg.nu_post);
  coarse_ = kernels::mg_coarse_plan(plan_.back().width, plan_.back().height, cfg.c_center, cfg.c_neighbor,
                                    cfg.coarse_reduction);
  lv_.resize(plan_.size());
  for (size_t k = 0; k < plan_.size(); ++k) {
    Level& l = lv_[k];
    l.geom = TileGeom::aligned(plan_[k].width, plan_[k].height, 1, 1, int(sizeof(T)));
    for (DeviceBuffer<T>* b : {&l.u[0], &l.u[1], &l.g}) {
      b->reset(l.geom.alloc_elems());
      MXS_HIP_CHECK(hipMemsetAsync(b->get(), 0, b->bytes(), stream_.get()));
    }
  }
  readback_.reset(lv_[0].geom);
  // The coarse solve once, outside any capture (it raises its LDS limit on
  // first use); g = 0 gives e = 0.
  Level& c = lv_.back();
  kernels::mg_coarse_solve<T>(c.g.get(), c.u[0].get(), c.geom, coarse_.table, 1, stream_.get());
  stream_.sync();
}

template <typename T>
void MultigridSolver<T>::set_boundary(const T* top, const T* bottom, const T* left, const T* right) {
  for (int k = 0; k < 2; ++k) copy_ring_sides(lv_[0].u[k].get(), lv_[0].geom, top, bottom, left, right, stream_.get());
  stream_.sync();
}

template <typename T>
void MultigridSolver<T>::set_source(const T* tile) {
  Level& l = lv_[0];
  if (tile) MXS_HIP_CHECK(hipMemcpyAsync(l.g.get(), tile, l.g.bytes(), hipMemcpyDeviceToDevice, stream_.get()));
  else MXS_HIP_CHECK(hipMemsetAsync(l.g.get(), 0, l.g.bytes(), stream_.get()));
  stream_.sync();
}

template <typename T>
void MultigridSolver<T>::set_field(const T* tile) {
  const TileGeom& g = lv_[0].geom;
  const index_t off = g.core_offset();
  MXS_HIP_CHECK(hipMemcpy2DAsync(lv_[0].u[0].get() + off, size_t(g.pitch) * sizeof(T), tile + off,
                                 size_t(g.pitch) * sizeof(T), size_t(g.width) * sizeof(T), size_t(g.height),
                                 hipMemcpyDeviceToDevice, stream_.get()));
  stream_.sync();
}

template <typename T>
void MultigridSolver<T>::field(T* tile) {
  MXS_HIP_CHECK(hipMemcpyAsync(tile, lv_[0].u[0].get(), lv_[0].u[0].bytes(), hipMemcpyDeviceToDevice, stream_.get()));
  stream_.sync();
}

template <typename T>
MultigridResidual MultigridSolver<T>::residual() {
  const Level& l = lv_[0];
  return readback_.template read<MultigridResidual>(l.u[0].get(), l.g.get(), l.geom, cfg_.c_center, cfg_.c_neighbor,
                                                    stream_);
}

template <typename T>
void MultigridSolver<T>::enqueue_level(size_t k) {
  Level& l = lv_[k];
  hipStream_t s = stream_.get();
  if (k + 1 == lv_.size()) {
    kernels::mg_coarse_solve<T>(l.g.get(), l.u[0].get(), l.geom, coarse_.table, coarse_.repeats, s);
    ++launches_;
    return;
  }
  Level& c = lv_[k + 1];
  const kernels::Stencil5Coeffs co{cfg_.c_center, cfg_.c_neighbor, false, -1.0};
  kernels::mg_smooth<T>(l.u[0].get(), l.u[1].get(), l.g.get(), l.geom, pre_, s);
  kernels::mg_residual_restrict<T>(l.u[1].get(), l.g.get(), l.geom, c.g.get(), c.geom, co, s);
  launches_ += 2;
  if (k + 2 < lv_.size()) {  // the coarse solve starts from 0 by itself
    MXS_HIP_CHECK(hipMemsetAsync(c.u[0].get(), 0, c.u[0].bytes(), s));
    ++launches_;
  }
  enqueue_level(k + 1);
  kernels::mg_prolong_add<T>(c.u[0].get(), c.geom, l.u[1].get(), l.geom, s);
  kernels::mg_smooth<T>(l.u[1].get(), l.u[0].get(), l.g.get(), l.geom, post_, s);
  launches_ += 2;
}

template <typename T>
void MultigridSolver<T>::enqueue_cycle() {
  launches_ = 0;
  enqueue_level(0);
}

template <typename T>
bool MultigridSolver<T>::capture() {
  graph_tried_ = true;
  return capture_linear(stream_, graph_, graph_status_, [&] { enqueue_cycle(); });
}

template <typename T>
void MultigridSolver<T>::vcycle(int n) {
  if (n < 0) throw std::invalid_argument("multigrid: vcycle(n) needs n >= 0");
  if (cfg_.graph && !graph_tried_) capture();
  for (int i = 0; i < n; ++i) {
    if (graph_.valid()) graph_.launch(stream_.get());
    else enqueue_cycle();
  }
  stream_.sync();
}

template <typename T>
MultigridSolve MultigridSolver<T>::solve(double tol, int max_cycles, const std::string& norm) {
  if (norm != "linf" && norm != "l2") throw std::invalid_argument("multigrid: norm must be 'linf' or 'l2', got '" + norm + "'");
  if (!(tol >= 0.0) || max_cycles < 0) throw std::invalid_argument("multigrid: solve needs tol >= 0 and max_cycles >= 0");
  MultigridSolve out;
  out.norm = norm;
  double best = 0.0;
  int since_best = 0;
  for (;;) {
    const MultigridResidual r = residual();
    out.residual = norm == "linf" ? r.linf : r.l2;
    out.history.push_back({out.cycles, r.linf, r.l2});
    if (!std::isfinite(out.residual) || !std::isfinite(r.linf)) {
      out.reason = "non-finite residual";
      break;
    }
    if (out.residual <= tol) {
      out.converged = true;
      out.reason = "converged: " + norm + " residual <= tol";
      break;
    }
    if (out.cycles == 0 || out.residual < best) {
      best = out.residual;
      since_best = 0;
    } else if (++since_best >= kMgStallCycles) {
      out.reason = "stalled";
      break;
    }
    if (out.cycles >= max_cycles) {
      out.reason = "max_cycles reached";
      break;
    }
    vcycle(1);
    ++out.cycles;
  }
  return out;
}

template <typename T>
std::string MultigridSolver<T>::note() const {
  std::ostringstream os;
  os << "multigrid V(" << cfg_.nu_pre << "," << cfg_.nu_post << "), " << plan_.size() << " levels " << plan_.front().width
     << "x" << plan_.front().height << " .. " << plan_.back().width << "x" << plan_.back().height << ", smoother omega "
     << cfg_.smoother_omega << ", coarse solve " << coarse_.repeats << " x " << coarse_.table.n
     << " Chebyshev sweeps (rho " << coarse_.rho << "), graph " << graph_status_;
  return os.str();
}

template class MultigridSolver<float>;
template class MultigridSolver<double>;

}  // namespace mxs
