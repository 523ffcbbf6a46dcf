// PcgSolver<T> (mxs/runtime/pcg_solver.hpp).
#include "mxs/runtime/pcg_solver.hpp"

#include <algorithm>
#include <sstream>

namespace mxs {

template <typename T>
PcgSolver<T>::PcgSolver(const PcgConfig& cfg)
    : CgSolverBase<T, kernels::PcgScalars>("preconditioned CG", cfg.c_center, cfg.c_neighbor, cfg.graph,
                                           kernels::ghost_sides_of(cfg.neumann)),
      cfg_(cfg) {
  plan_ = kernels::pcg_plan_levels(cfg.width, cfg.height, cfg.c_center, cfg.c_neighbor, this->sides_);
  coarse_ = kernels::pcg_coarse_plan(plan_.back(), cfg.c_neighbor, cfg.coarse_reduction);
  this->allocate(cfg.width, cfg.height);
  hipStream_t s = this->stream_.get();
  lv_.resize(plan_.size());
  for (size_t k = 0; k < plan_.size(); ++k) {
    Level& l = lv_[k];
    l.geom = TileGeom::aligned(plan_[k].width, plan_[k].height, 1, 1, int(sizeof(T)));
    l.smooth = kernels::mg_smoother_table(plan_[k].c0, cfg.c_neighbor, cfg.smoother_omega, cfg.nu);
    for (DeviceBuffer<T>* b : {&l.u[0], &l.u[1], &l.g}) {
      if (k == 0 && b == &l.g) continue;
      b->reset(l.geom.alloc_elems());
      MXS_HIP_CHECK(hipMemsetAsync(b->get(), 0, b->bytes(), s));
    }
  }
  // The smoother's dot epilogue reduces over the same partials.
  this->partials_.reset(
      2 * index_t(std::max(kernels::cg_grid_size(this->geom_), kernels::mgp_smooth_grid_size(this->geom_))));
  // The coarse solve once, outside any capture (it raises its LDS limit on
  // first use); a source of 0 gives e = 0.
  Level& c = lv_.back();
  kernels::mgp_coarse_solve<T>(lv_.size() == 1 ? this->r_.get() : c.g.get(), c.u[0].get(), c.geom, coarse_.table, 1,
                               plan_.back().sides, nullptr, s);
  this->stream_.sync();
}

template <typename T>
void PcgSolver<T>::launch_start(bool into_scratch) {
  hipStream_t s = this->stream_.get();
  // The first direction of a run is fma(0, p_old, z): p_old has to be finite.
  if (!into_scratch) MXS_HIP_CHECK(hipMemsetAsync(this->p_[0].get(), 0, this->p_[0].bytes(), s));
  kernels::pcg_start<T>(this->u_.get(), this->g_.get(), (into_scratch ? this->q_ : this->r_).get(), this->geom_,
                        this->coeffs(), (into_scratch ? this->residual_scalars_ : this->scalars_).get(),
                        this->partials_.get(), this->counter_.get(), s, this->sides_);
}

template <typename T>
void PcgSolver<T>::launch_heat_start(const kernels::HeatCoeffs& hc, const T* q) {
  hipStream_t s = this->stream_.get();
  MXS_HIP_CHECK(hipMemsetAsync(this->p_[0].get(), 0, this->p_[0].bytes(), s));  // as launch_start
  kernels::pcg_heat_start<T>(this->u_.get(), q, this->g_.get(), this->r_.get(), this->geom_, hc, this->scalars_.get(),
                             this->partials_.get(), this->counter_.get(), s, this->sides_);
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
  hipStream_t s = this->stream_.get();
  const T* src = k == 0 ? this->r_.get() : l.g.get();
  kernels::PcgScalars* dot = k == 0 ? this->scalars_.get() : nullptr;
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
                         dot ? this->partials_.get() : nullptr, dot ? this->counter_.get() : nullptr, s);
  launches_ += 2;
}

template <typename T>
void PcgSolver<T>::enqueue_iterations(int n, int parity) {
  hipStream_t s = this->stream_.get();
  const kernels::Stencil5Coeffs c = this->coeffs();
  auto& p = this->p_;
  T* z = lv_[0].u[0].get();
  for (int i = 0; i < n; ++i) {
    const int a = (parity + i) & 1;
    launches_ = 0;
    enqueue_level(0);
    kernels::pcg_apply<T>(z, p[a].get(), p[a ^ 1].get(), this->q_.get(), this->geom_, c, this->scalars_.get(),
                          this->partials_.get(), this->counter_.get(), s, this->sides_);
    kernels::pcg_update<T>(this->u_.get(), this->r_.get(), p[a ^ 1].get(), this->q_.get(), this->geom_,
                           this->scalars_.get(), this->partials_.get(), this->counter_.get(), s);
    launches_ += 2;
  }
}

template <typename T>
std::string PcgSolver<T>::note() const {
  std::ostringstream os;
  os << "multigrid-preconditioned CG " << cfg_.width << "x" << cfg_.height << ", c_center " << cfg_.c_center
     << ", c_neighbor " << cfg_.c_neighbor
     << (this->sides_.any_mirror() ? ", Neumann sides " + kernels::ghost_sides_names(this->sides_) : std::string())
     << ", V(" << cfg_.nu << "," << cfg_.nu << ") over " << plan_.size() << " levels down to " << plan_.back().width
     << "x" << plan_.back().height << ", smoother omega " << cfg_.smoother_omega << ", coarse solve " << coarse_.repeats
     << " x " << coarse_.table.n << " Chebyshev sweeps (rho " << coarse_.rho << "), graph " << this->graph_status_;
  if (this->graph_.valid()) os << " (" << this->graph_iters_ << " iterations per launch)";
  return os.str();
}

template class PcgSolver<float>;
template class PcgSolver<double>;

}  // namespace mxs
