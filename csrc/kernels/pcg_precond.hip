// Launchers of the V-cycle preconditioner's kernels (kernels.hpp; device code
// in pcg_device.hpp): stream-ordered, allocation-free and synchronisation-free,
// so a block of PCG iterations captures into one linear hipGraph.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "mxs/core/error.hpp"
#include "mxs/kernels/kernels.hpp"
#include "pcg_device.hpp"

namespace mxs {
namespace kernels {
namespace {

std::atomic<const char*> g_last_pcg{""};

void check_tile(const TileGeom& g, const char* who) {
  MXS_CHECK(g.halo_x >= 1 && g.halo_y >= 1, who << ": the tile has no ghost ring (it needs one at least 1 deep)");
  MXS_CHECK(g.width >= 1 && g.height >= 1 && g.pitch >= g.x_origin + g.total_width(), who << ": bad tile geometry");
}

void check_pair(const TileGeom& g, const TileGeom& gc, const char* who) {
  check_tile(g, who);
  check_tile(gc, who);
  MXS_CHECK(g.width >= 2 && g.height >= 2 && gc.width == g.width / 2 && gc.height == g.height / 2,
            who << ": the coarse tile must be (width / 2) x (height / 2) of a fine tile with both sides >= 2; got "
                << g.width << " x " << g.height << " -> " << gc.width << " x " << gc.height);
}

template <typename T, int N>
detail::MgSweeps<T, N> sweeps_of(const MgSweepTable& t) {
  detail::MgSweeps<T, N> k{};
  for (int l = 0; l < N; ++l) {
    const int j = l < t.n ? l : t.n - 1;
    k.center[l] = T(t.center[j]);
    k.neighbor[l] = T(t.neighbor[j]);
    k.weight[l] = T(t.weight[j]);
  }
  return k;
}

// A level's codes: near sides ring or mirror, far sides also reflect.
detail::MgpSides sides_of(const GhostSides& sd, const char* who) {
  MXS_CHECK((sd.top == kGhostRing || sd.top == kGhostMirror) && (sd.left == kGhostRing || sd.left == kGhostMirror),
            who << ": a near side (top, left) is ring (0) or mirror (+1)");
  MXS_CHECK(sd.bottom >= -1 && sd.bottom <= 1 && sd.right >= -1 && sd.right <= 1,
            who << ": a far side (bottom, right) is ring (0), mirror (+1) or reflect (-1)");
  return detail::MgpSides{sd.top, sd.bottom, sd.left, sd.right};
}

dim3 smooth_grid(const TileGeom& g) {
  return dim3(unsigned((g.width + detail::kMgTw - 1) / detail::kMgTw),
              unsigned((g.height + detail::kMgTh - 1) / detail::kMgTh));
}

template <typename T, int NU>
void launch_smooth(const T* in, T* out, const T* src, const TileGeom& g, const MgSweepTable& t, detail::MgpSides sd,
                   PcgScalars* sc, double* partials, unsigned* counter, hipStream_t s) {
  const dim3 grid = smooth_grid(g);
  PcgScalars* no_sc = nullptr;
  double* no_partials = nullptr;
  unsigned* no_counter = nullptr;
  if (sc)  // the finest post-smooth: never from zero
    detail::mgp_smooth_kernel<T, NU, true, false><<<grid, detail::kMgBlock, 0, s>>>(
        in, out, src, g.pitch, g.core_offset(), g.width, g.height, sweeps_of<T, NU>(t), sd, sc, partials, counter);
  else if (in == nullptr)
    detail::mgp_smooth_kernel<T, NU, false, true><<<grid, detail::kMgBlock, 0, s>>>(
        in, out, src, g.pitch, g.core_offset(), g.width, g.height, sweeps_of<T, NU>(t), sd, no_sc, no_partials,
        no_counter);
  else
    detail::mgp_smooth_kernel<T, NU, false, false><<<grid, detail::kMgBlock, 0, s>>>(
        in, out, src, g.pitch, g.core_offset(), g.width, g.height, sweeps_of<T, NU>(t), sd, no_sc, no_partials,
        no_counter);
}

}  // namespace

const char* last_pcg_dispatch() { return g_last_pcg.load(); }

int mgp_smooth_grid_size(const TileGeom& g) {
  const dim3 grid = smooth_grid(g);
  return int(grid.x * grid.y);
}

template <typename T>
void mgp_smooth(const T* u_in, T* u_out, const T* src, const TileGeom& g, const MgSweepTable& t, GhostSides sides,
                PcgScalars* scalars, double* partials, unsigned* counter, hipStream_t s) {
  check_tile(g, "mgp_smooth");
  const detail::MgpSides sd = sides_of(sides, "mgp_smooth");
  MXS_CHECK(t.n >= 1 && t.n <= kMgMaxSmooth, "mgp_smooth: 1.." << kMgMaxSmooth << " sweeps per launch, got " << t.n);
  MXS_CHECK(u_out && src && u_in != u_out, "mgp_smooth: needs u_out and src, u_in != u_out");
  MXS_CHECK(u_in || !scalars, "mgp_smooth: a start from zero (u_in null) carries no dot epilogue");
  MXS_CHECK((g.height + detail::kMgTh - 1) / detail::kMgTh <= 65535, "mgp_smooth: too many tile rows for one launch");
  MXS_CHECK((scalars != nullptr) == (partials != nullptr) && (scalars != nullptr) == (counter != nullptr),
            "mgp_smooth: the dot epilogue needs the scalar block, the partials and the ticket together");
  if (scalars)
    MXS_CHECK(reinterpret_cast<std::uintptr_t>(scalars) % sizeof(double) == 0 &&
                  reinterpret_cast<std::uintptr_t>(partials) % sizeof(double) == 0 &&
                  reinterpret_cast<std::uintptr_t>(counter) % sizeof(unsigned) == 0,
              "mgp_smooth: the scalar block, the partials and the ticket must be aligned");
  switch (t.n) {
    case 1: launch_smooth<T, 1>(u_in, u_out, src, g, t, sd, scalars, partials, counter, s); break;
    case 2: launch_smooth<T, 2>(u_in, u_out, src, g, t, sd, scalars, partials, counter, s); break;
    case 3: launch_smooth<T, 3>(u_in, u_out, src, g, t, sd, scalars, partials, counter, s); break;
    default: launch_smooth<T, 4>(u_in, u_out, src, g, t, sd, scalars, partials, counter, s); break;
  }
  g_last_pcg = scalars ? "mgp_smooth_dot" : (u_in ? "mgp_smooth" : "mgp_smooth_zero");
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void mgp_residual_restrict(const T* u, const T* src, const TileGeom& g, GhostSides sides, T* coarse_src,
                           const TileGeom& gc, Stencil5Coeffs c, hipStream_t s) {
  check_pair(g, gc, "mgp_residual_restrict");
  const detail::MgpSides sd = sides_of(sides, "mgp_residual_restrict");
  MXS_CHECK(u && src && coarse_src, "mgp_residual_restrict: needs u, src and coarse_src");
  const dim3 grid(unsigned((gc.width + detail::kMgCw - 1) / detail::kMgCw),
                  unsigned((gc.height + detail::kMgCh - 1) / detail::kMgCh));
  MXS_CHECK(grid.y <= 65535, "mgp_residual_restrict: too many tile rows for one launch");
  detail::mgp_residual_restrict_kernel<T><<<grid, detail::kMgBlock, 0, s>>>(
      u, src, g.pitch, g.core_offset(), g.width, g.height, sd, coarse_src, gc.pitch, gc.core_offset(), gc.width,
      gc.height, T(c.center), T(c.neighbor));
  g_last_pcg = "mgp_residual_restrict";
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void mgp_prolong_add(const T* e, const TileGeom& gc, T* u, const TileGeom& g, hipStream_t s, GhostSides sides) {
  check_pair(g, gc, "mgp_prolong_add");
  const detail::MgpSides sd = sides_of(sides, "mgp_prolong_add");
  MXS_CHECK(e && u, "mgp_prolong_add: needs e and u");
  const dim3 grid(unsigned((g.width + 63) / 64), unsigned((g.height + 3) / 4));
  MXS_CHECK(grid.y <= 65535, "mgp_prolong_add: too many rows for one launch");
  detail::mgp_prolong_add_kernel<T><<<grid, detail::kMgBlock, 0, s>>>(
      e, gc.pitch, gc.core_offset(), gc.width, gc.height, u, g.pitch, g.core_offset(), g.width, g.height, sd);
  g_last_pcg = "mgp_prolong_add";
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void mgp_coarse_solve(const T* src, T* e, const TileGeom& g, const MgSweepTable& t, int repeats, GhostSides sides,
                      PcgScalars* scalars, hipStream_t s) {
  check_tile(g, "mgp_coarse_solve");
  const detail::MgpSides sd = sides_of(sides, "mgp_coarse_solve");
  MXS_CHECK(reinterpret_cast<std::uintptr_t>(scalars) % sizeof(double) == 0, "mgp_coarse_solve: the scalar block must be aligned");
  MXS_CHECK(g.width <= kMgCoarsestMax && g.height <= kMgCoarsestMax,
            "mgp_coarse_solve: the grid must be at most " << kMgCoarsestMax << " on both sides, got " << g.width << " x "
                                                          << g.height);
  MXS_CHECK(t.n >= 1 && t.n <= kMaxLevels && repeats >= 1 && repeats <= kMgMaxCoarseRepeats,
            "mgp_coarse_solve: 1.." << kMaxLevels << " levels, 1.." << kMgMaxCoarseRepeats << " repeats");
  MXS_CHECK(src && e, "mgp_coarse_solve: needs src and e");
  const size_t lds = size_t(2 * (g.width + 2) * (g.height + 2) + g.width * g.height) * sizeof(T);
  // Above the 64 KiB default the kernel has to be told once (per element type).
  static bool raised = false;
  if (!raised) {
    const size_t most = size_t(2 * (kMgCoarsestMax + 2) * (kMgCoarsestMax + 2) + kMgCoarsestMax * kMgCoarsestMax) * sizeof(T);
    MXS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(detail::mgp_coarse_solve_kernel<T>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, int(most)));
    raised = true;
  }
  detail::mgp_coarse_solve_kernel<T><<<1, detail::kMgBlock, lds, s>>>(src, e, g.pitch, g.core_offset(), int(g.width),
                                                                      int(g.height), repeats,
                                                                      sweeps_of<T, kMaxLevels>(t), t.n, sd, scalars);
  g_last_pcg = "mgp_coarse_solve";
  MXS_HIP_CHECK_LAUNCH();
}

#define MXS_MGP_INSTANTIATE(T)                                                                                        \
  template void mgp_smooth<T>(const T*, T*, const T*, const TileGeom&, const MgSweepTable&, GhostSides, PcgScalars*, \
                              double*, unsigned*, hipStream_t);                                                      \
  template void mgp_residual_restrict<T>(const T*, const T*, const TileGeom&, GhostSides, T*, const TileGeom&,       \
                                         Stencil5Coeffs, hipStream_t);                                               \
  template void mgp_prolong_add<T>(const T*, const TileGeom&, T*, const TileGeom&, hipStream_t, GhostSides);          \
  template void mgp_coarse_solve<T>(const T*, T*, const TileGeom&, const MgSweepTable&, int, GhostSides, PcgScalars*, \
                                    hipStream_t);
MXS_MGP_INSTANTIATE(float)
MXS_MGP_INSTANTIATE(double)
#undef MXS_MGP_INSTANTIATE

}  // namespace kernels
}  // namespace mxs
