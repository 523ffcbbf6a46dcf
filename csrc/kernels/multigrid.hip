// Launchers of the multigrid kernels (kernels.hpp; device code in
// multigrid_device.hpp): stream-ordered, allocation-free and
// synchronisation-free, so a whole V-cycle captures into one linear hipGraph.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "mxs/core/error.hpp"
#include "mxs/kernels/kernels.hpp"
#include "multigrid_device.hpp"

namespace mxs {
namespace kernels {
namespace {

std::atomic<const char*> g_last_mg{""};

void check_tile(const TileGeom& g, const char* who) {
  MXS_CHECK(g.halo_x >= 1 && g.halo_y >= 1, who << ": the tile has no ghost ring (it needs one at least 1 deep)");
  MXS_CHECK(g.width >= 1 && g.height >= 1 && g.pitch >= g.x_origin + g.total_width(), who << ": bad tile geometry");
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

template <typename T, int NU>
void launch_smooth(const T* in, T* out, const T* src, const TileGeom& g, const MgSweepTable& t, hipStream_t s) {
  const dim3 grid(unsigned((g.width + detail::kMgTw - 1) / detail::kMgTw),
                  unsigned((g.height + detail::kMgTh - 1) / detail::kMgTh));
  detail::mg_smooth_kernel<T, NU><<<grid, detail::kMgBlock, 0, s>>>(in, out, src, g.pitch, g.core_offset(), g.width,
                                                                    g.height, sweeps_of<T, NU>(t));
}

}  // namespace

const char* last_multigrid_dispatch() { return g_last_mg.load(); }

template <typename T>
void mg_smooth(const T* u_in, T* u_out, const T* src, const TileGeom& g, const MgSweepTable& t, hipStream_t s) {
  check_tile(g, "mg_smooth");
  MXS_CHECK(t.n >= 1 && t.n <= kMgMaxSmooth, "mg_smooth: 1.." << kMgMaxSmooth << " sweeps per launch, got " << t.n);
  MXS_CHECK(u_in && u_out && src && u_in != u_out, "mg_smooth: needs u_in, u_out and src, u_in != u_out");
  MXS_CHECK((g.height + detail::kMgTh - 1) / detail::kMgTh <= 65535, "mg_smooth: too many tile rows for one launch");
  switch (t.n) {
    case 1: launch_smooth<T, 1>(u_in, u_out, src, g, t, s); break;
    case 2: launch_smooth<T, 2>(u_in, u_out, src, g, t, s); break;
    case 3: launch_smooth<T, 3>(u_in, u_out, src, g, t, s); break;
    default: launch_smooth<T, 4>(u_in, u_out, src, g, t, s); break;
  }
  g_last_mg = "mg_smooth";
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void mg_residual_restrict(const T* u, const T* src, const TileGeom& g, T* coarse_src, const TileGeom& gc,
                          Stencil5Coeffs c, hipStream_t s) {
  check_tile(g, "mg_residual_restrict");
  check_tile(gc, "mg_residual_restrict (coarse)");
  MXS_CHECK(g.width == 2 * gc.width + 1 && g.height == 2 * gc.height + 1,
            "mg_residual_restrict: the coarse tile must be ((width - 1) / 2) x ((height - 1) / 2) of an odd fine tile; got "
                << g.width << " x " << g.height << " -> " << gc.width << " x " << gc.height);
  MXS_CHECK(u && src && coarse_src, "mg_residual_restrict: needs u, src and coarse_src");
  const dim3 grid(unsigned((gc.width + detail::kMgCw - 1) / detail::kMgCw),
                  unsigned((gc.height + detail::kMgCh - 1) / detail::kMgCh));
  MXS_CHECK(grid.y <= 65535, "mg_residual_restrict: too many tile rows for one launch");
  detail::mg_residual_restrict_kernel<T><<<grid, detail::kMgBlock, 0, s>>>(
      u, src, g.pitch, g.core_offset(), g.width, g.height, coarse_src, gc.pitch, gc.core_offset(), gc.width, gc.height,
      T(c.center), T(c.neighbor));
  g_last_mg = "mg_residual_restrict";
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void mg_prolong_add(const T* e, const TileGeom& gc, T* u, const TileGeom& g, hipStream_t s) {
  check_tile(g, "mg_prolong_add");
  check_tile(gc, "mg_prolong_add (coarse)");
  MXS_CHECK(g.width == 2 * gc.width + 1 && g.height == 2 * gc.height + 1,
            "mg_prolong_add: the coarse tile must be ((width - 1) / 2) x ((height - 1) / 2) of an odd fine tile; got "
                << g.width << " x " << g.height << " -> " << gc.width << " x " << gc.height);
  MXS_CHECK(e && u, "mg_prolong_add: needs e and u");
  const dim3 grid(unsigned((g.width + 63) / 64), unsigned((g.height + 3) / 4));
  MXS_CHECK(grid.y <= 65535, "mg_prolong_add: too many rows for one launch");
  detail::mg_prolong_add_kernel<T><<<grid, detail::kMgBlock, 0, s>>>(e, gc.pitch, gc.core_offset(), gc.width, gc.height,
                                                                     u, g.pitch, g.core_offset(), g.width, g.height);
  g_last_mg = "mg_prolong_add";
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void mg_coarse_solve(const T* src, T* e, const TileGeom& g, const MgSweepTable& t, int repeats, hipStream_t s) {
  check_tile(g, "mg_coarse_solve");
  MXS_CHECK(g.width <= kMgCoarsestMax && g.height <= kMgCoarsestMax,
            "mg_coarse_solve: the grid must be at most " << kMgCoarsestMax << " on both sides, got " << g.width << " x "
                                                         << g.height);
  MXS_CHECK(t.n >= 1 && t.n <= kMaxLevels && repeats >= 1 && repeats <= kMgMaxCoarseRepeats,
            "mg_coarse_solve: 1.." << kMaxLevels << " levels, 1.." << kMgMaxCoarseRepeats << " repeats");
  MXS_CHECK(src && e, "mg_coarse_solve: needs src and e");
  const size_t lds = size_t(2 * (g.width + 2) * (g.height + 2) + g.width * g.height) * sizeof(T);
  // Above the 64 KiB default the kernel has to be told once (per element type).
  static bool raised = false;
  if (!raised) {
    const size_t most = size_t(2 * (kMgCoarsestMax + 2) * (kMgCoarsestMax + 2) + kMgCoarsestMax * kMgCoarsestMax) * sizeof(T);
    MXS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(detail::mg_coarse_solve_kernel<T>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, int(most)));
    raised = true;
  }
  detail::mg_coarse_solve_kernel<T><<<1, detail::kMgBlock, lds, s>>>(src, e, g.pitch, g.core_offset(), int(g.width),
                                                                     int(g.height), repeats,
                                                                     sweeps_of<T, kMaxLevels>(t), t.n);
  g_last_mg = "mg_coarse_solve";
  MXS_HIP_CHECK_LAUNCH();
}

#define MXS_MG_INSTANTIATE(T)                                                                                         \
  template void mg_smooth<T>(const T*, T*, const T*, const TileGeom&, const MgSweepTable&, hipStream_t);              \
  template void mg_residual_restrict<T>(const T*, const T*, const TileGeom&, T*, const TileGeom&, Stencil5Coeffs,     \
                                        hipStream_t);                                                                 \
  template void mg_prolong_add<T>(const T*, const TileGeom&, T*, const TileGeom&, hipStream_t);                       \
  template void mg_coarse_solve<T>(const T*, T*, const TileGeom&, const MgSweepTable&, int, hipStream_t);
MXS_MG_INSTANTIATE(float)
MXS_MG_INSTANTIATE(double)
#undef MXS_MG_INSTANTIATE

}  // namespace kernels
}  // namespace mxs
