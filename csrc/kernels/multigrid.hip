// Launchers of the multigrid kernels, the solver's (mg_*) and the V-cycle
// preconditioner's (mgp_*) (kernels.hpp; device code in multigrid_device.hpp):
// stream-ordered, allocation-free and synchronisation-free, so a whole V-cycle
// or a block of PCG iterations captures into one linear hipGraph. Each public
// entry makes its own checks and then runs the launch the two share.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <type_traits>

#include "mxs/core/error.hpp"
#include "mxs/kernels/kernels.hpp"
#include "multigrid_device.hpp"

namespace mxs {
namespace kernels {
namespace {

std::atomic<const char*> g_last_mg{""};
std::atomic<const char*> g_last_pcg{""};

void check_tile(const TileGeom& g, const char* who) {
  MXS_CHECK(g.halo_x >= 1 && g.halo_y >= 1, who << ": the tile has no ghost ring (it needs one at least 1 deep)");
  MXS_CHECK(g.width >= 1 && g.height >= 1 && g.pitch >= g.x_origin + g.total_width(), who << ": bad tile geometry");
}

// The solver's level rule: an odd fine tile over ((width - 1) / 2) x ((height - 1) / 2).
void check_odd_pair(const TileGeom& g, const TileGeom& gc, const char* who, const char* who_coarse) {
  check_tile(g, who);
  check_tile(gc, who_coarse);
  MXS_CHECK(g.width == 2 * gc.width + 1 && g.height == 2 * gc.height + 1,
            who << ": the coarse tile must be ((width - 1) / 2) x ((height - 1) / 2) of an odd fine tile; got "
                << g.width << " x " << g.height << " -> " << gc.width << " x " << gc.height);
}

// The preconditioner's: any fine tile over (width / 2) x (height / 2).
void check_half_pair(const TileGeom& g, const TileGeom& gc, const char* who) {
  check_tile(g, who);
  check_tile(gc, who);
  MXS_CHECK(g.width >= 2 && g.height >= 2 && gc.width == g.width / 2 && gc.height == g.height / 2,
            who << ": the coarse tile must be (width / 2) x (height / 2) of a fine tile with both sides >= 2; got "
                << g.width << " x " << g.height << " -> " << gc.width << " x " << gc.height);
}

// A level's codes: near sides ring or mirror, far sides also reflect.
detail::MgpSides sides_of(const GhostSides& sd, const char* who) {
  MXS_CHECK((sd.top == kGhostRing || sd.top == kGhostMirror) && (sd.left == kGhostRing || sd.left == kGhostMirror),
            who << ": a near side (top, left) is ring (0) or mirror (+1)");
  MXS_CHECK(sd.bottom >= -1 && sd.bottom <= 1 && sd.right >= -1 && sd.right <= 1,
            who << ": a far side (bottom, right) is ring (0), mirror (+1) or reflect (-1)");
  return detail::MgpSides{sd.top, sd.bottom, sd.left, sd.right};
}

// A launch's table: the sweeps rounded to T, alone or with the preconditioner's extras.
template <typename T, int N>
detail::MgSweeps<T, N> table_of(const MgSweepTable& t, detail::MgNoExtras) {
  detail::MgSweeps<T, N> k{};
  for (int l = 0; l < N; ++l) {
    const int j = l < t.n ? l : t.n - 1;
    k.center[l] = T(t.center[j]);
    k.neighbor[l] = T(t.neighbor[j]);
    k.weight[l] = T(t.weight[j]);
  }
  return k;
}
template <typename T, int N>
detail::MgpSweeps<T, N> table_of(const MgSweepTable& t, const detail::MgpExtras& x) {
  return detail::MgpSweeps<T, N>{table_of<T, N>(t, detail::MgNoExtras{}), x};
}

dim3 smooth_grid(const TileGeom& g) {
  return dim3(unsigned((g.width + detail::kMgTw - 1) / detail::kMgTw),
              unsigned((g.height + detail::kMgTh - 1) / detail::kMgTh));
}

void check_smooth(const TileGeom& g, const MgSweepTable& t, const char* who) {
  check_tile(g, who);
  MXS_CHECK(t.n >= 1 && t.n <= kMgMaxSmooth, who << ": 1.." << kMgMaxSmooth << " sweeps per launch, got " << t.n);
  MXS_CHECK(smooth_grid(g).y <= 65535, who << ": too many tile rows for one launch");
}

template <typename T, bool DOT, bool ZERO, typename Extras>
void launch_smooth(const T* in, T* out, const T* src, const TileGeom& g, const MgSweepTable& t, const Extras& x,
                   hipStream_t s) {
  auto launch = [&](auto nu) {
    constexpr int NU = decltype(nu)::value;
    detail::mg_smooth_kernel<T, NU, DOT, ZERO><<<smooth_grid(g), detail::kMgBlock, 0, s>>>(
        in, out, src, g.pitch, g.core_offset(), g.width, g.height, table_of<T, NU>(t, x));
  };
  switch (t.n) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    default: launch(std::integral_constant<int, 4>{}); break;
  }
}

// `sd`: the preconditioner's MgpSides, or nothing (the kernels' Sides pack).
template <typename T, typename... Sides>
void launch_residual_restrict(const T* u, const T* src, const TileGeom& g, T* coarse_src, const TileGeom& gc,
                              Stencil5Coeffs c, const char* who, hipStream_t s, Sides... sd) {
  MXS_CHECK(u && src && coarse_src, who << ": needs u, src and coarse_src");
  const dim3 grid(unsigned((gc.width + detail::kMgCw - 1) / detail::kMgCw),
                  unsigned((gc.height + detail::kMgCh - 1) / detail::kMgCh));
  MXS_CHECK(grid.y <= 65535, who << ": too many tile rows for one launch");
  detail::mg_residual_restrict_kernel<T, Sides...><<<grid, detail::kMgBlock, 0, s>>>(
      u, src, g.pitch, g.core_offset(), g.width, g.height, sd..., coarse_src, gc.pitch, gc.core_offset(), gc.width,
      gc.height, T(c.center), T(c.neighbor));
}

template <typename T, typename... Sides>
void launch_prolong_add(const T* e, const TileGeom& gc, T* u, const TileGeom& g, const char* who, hipStream_t s,
                        Sides... sd) {
  MXS_CHECK(e && u, who << ": needs e and u");
  const dim3 grid(unsigned((g.width + 63) / 64), unsigned((g.height + 3) / 4));
  MXS_CHECK(grid.y <= 65535, who << ": too many rows for one launch");
  detail::mg_prolong_add_kernel<T, Sides...><<<grid, detail::kMgBlock, 0, s>>>(
      e, gc.pitch, gc.core_offset(), gc.width, gc.height, u, g.pitch, g.core_offset(), g.width, g.height, sd...);
}

template <typename T, typename Extras>
void launch_coarse_solve(const T* src, T* e, const TileGeom& g, const MgSweepTable& t, int repeats, const Extras& x,
                         const char* who, hipStream_t s) {
  MXS_CHECK(g.width <= kMgCoarsestMax && g.height <= kMgCoarsestMax,
            who << ": the grid must be at most " << kMgCoarsestMax << " on both sides, got " << g.width << " x "
                << g.height);
  MXS_CHECK(t.n >= 1 && t.n <= kMaxLevels && repeats >= 1 && repeats <= kMgMaxCoarseRepeats,
            who << ": 1.." << kMaxLevels << " levels, 1.." << kMgMaxCoarseRepeats << " repeats");
  MXS_CHECK(src && e, who << ": needs src and e");
  const auto tab = table_of<T, kMaxLevels>(t, x);
  const auto kernel = detail::mg_coarse_solve_kernel<T, std::remove_const_t<decltype(tab)>>;
  const auto lds_of = [](index_t w, index_t h) { return size_t(2 * (w + 2) * (h + 2) + w * h) * sizeof(T); };
  // Above the 64 KiB default the kernel has to be told once: this flag is one
  // per instantiation of this function, which is one per kernel.
  static bool raised = false;
  if (!raised) {
    MXS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      int(lds_of(kMgCoarsestMax, kMgCoarsestMax))));
    raised = true;
  }
  kernel<<<1, detail::kMgBlock, lds_of(g.width, g.height), s>>>(src, e, g.pitch, g.core_offset(), int(g.width),
                                                                int(g.height), repeats, tab, t.n);
}

}  // namespace

const char* last_multigrid_dispatch() { return g_last_mg.load(); }
const char* last_pcg_dispatch() { return g_last_pcg.load(); }

int mgp_smooth_grid_size(const TileGeom& g) {
  const dim3 grid = smooth_grid(g);
  return int(grid.x * grid.y);
}

template <typename T>
void mg_smooth(const T* u_in, T* u_out, const T* src, const TileGeom& g, const MgSweepTable& t, hipStream_t s) {
  check_smooth(g, t, "mg_smooth");
  MXS_CHECK(u_in && u_out && src && u_in != u_out, "mg_smooth: needs u_in, u_out and src, u_in != u_out");
  launch_smooth<T, false, false>(u_in, u_out, src, g, t, detail::MgNoExtras{}, s);
  g_last_mg = "mg_smooth";
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void mgp_smooth(const T* u_in, T* u_out, const T* src, const TileGeom& g, const MgSweepTable& t, GhostSides sides,
                PcgScalars* scalars, double* partials, unsigned* counter, hipStream_t s) {
  check_smooth(g, t, "mgp_smooth");
  const detail::MgpExtras x{sides_of(sides, "mgp_smooth"), scalars, partials, counter};
  MXS_CHECK(u_out && src && u_in != u_out, "mgp_smooth: needs u_out and src, u_in != u_out");
  MXS_CHECK(u_in || !scalars, "mgp_smooth: a start from zero (u_in null) carries no dot epilogue");
  MXS_CHECK((scalars != nullptr) == (partials != nullptr) && (scalars != nullptr) == (counter != nullptr),
            "mgp_smooth: the dot epilogue needs the scalar block, the partials and the ticket together");
  if (scalars)
    MXS_CHECK(reinterpret_cast<std::uintptr_t>(scalars) % sizeof(double) == 0 &&
                  reinterpret_cast<std::uintptr_t>(partials) % sizeof(double) == 0 &&
                  reinterpret_cast<std::uintptr_t>(counter) % sizeof(unsigned) == 0,
              "mgp_smooth: the scalar block, the partials and the ticket must be aligned");
  if (scalars) launch_smooth<T, true, false>(u_in, u_out, src, g, t, x, s);  // the finest post-smooth: never from zero
  else if (!u_in) launch_smooth<T, false, true>(u_in, u_out, src, g, t, x, s);
  else launch_smooth<T, false, false>(u_in, u_out, src, g, t, x, s);
  g_last_pcg = scalars ? "mgp_smooth_dot" : (u_in ? "mgp_smooth" : "mgp_smooth_zero");
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void mg_residual_restrict(const T* u, const T* src, const TileGeom& g, T* coarse_src, const TileGeom& gc,
                          Stencil5Coeffs c, hipStream_t s) {
  check_odd_pair(g, gc, "mg_residual_restrict", "mg_residual_restrict (coarse)");
  launch_residual_restrict(u, src, g, coarse_src, gc, c, "mg_residual_restrict", s);
  g_last_mg = "mg_residual_restrict";
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void mgp_residual_restrict(const T* u, const T* src, const TileGeom& g, GhostSides sides, T* coarse_src,
                           const TileGeom& gc, Stencil5Coeffs c, hipStream_t s) {
  check_half_pair(g, gc, "mgp_residual_restrict");
  launch_residual_restrict(u, src, g, coarse_src, gc, c, "mgp_residual_restrict", s,
                           sides_of(sides, "mgp_residual_restrict"));
  g_last_pcg = "mgp_residual_restrict";
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void mg_prolong_add(const T* e, const TileGeom& gc, T* u, const TileGeom& g, hipStream_t s) {
  check_odd_pair(g, gc, "mg_prolong_add", "mg_prolong_add (coarse)");
  launch_prolong_add(e, gc, u, g, "mg_prolong_add", s);
  g_last_mg = "mg_prolong_add";
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void mgp_prolong_add(const T* e, const TileGeom& gc, T* u, const TileGeom& g, hipStream_t s, GhostSides sides) {
  check_half_pair(g, gc, "mgp_prolong_add");
  launch_prolong_add(e, gc, u, g, "mgp_prolong_add", s, sides_of(sides, "mgp_prolong_add"));
  g_last_pcg = "mgp_prolong_add";
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void mg_coarse_solve(const T* src, T* e, const TileGeom& g, const MgSweepTable& t, int repeats, hipStream_t s) {
  check_tile(g, "mg_coarse_solve");
  launch_coarse_solve(src, e, g, t, repeats, detail::MgNoExtras{}, "mg_coarse_solve", s);
  g_last_mg = "mg_coarse_solve";
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void mgp_coarse_solve(const T* src, T* e, const TileGeom& g, const MgSweepTable& t, int repeats, GhostSides sides,
                      PcgScalars* scalars, hipStream_t s) {
  check_tile(g, "mgp_coarse_solve");
  const detail::MgpExtras x{sides_of(sides, "mgp_coarse_solve"), scalars, nullptr, nullptr};
  MXS_CHECK(reinterpret_cast<std::uintptr_t>(scalars) % sizeof(double) == 0, "mgp_coarse_solve: the scalar block must be aligned");
  launch_coarse_solve(src, e, g, t, repeats, x, "mgp_coarse_solve", s);
  g_last_pcg = "mgp_coarse_solve";
  MXS_HIP_CHECK_LAUNCH();
}

#define MXS_MG_INSTANTIATE(T)                                                                                         \
  template void mg_smooth<T>(const T*, T*, const T*, const TileGeom&, const MgSweepTable&, hipStream_t);              \
  template void mg_residual_restrict<T>(const T*, const T*, const TileGeom&, T*, const TileGeom&, Stencil5Coeffs,     \
                                        hipStream_t);                                                                 \
  template void mg_prolong_add<T>(const T*, const TileGeom&, T*, const TileGeom&, hipStream_t);                       \
  template void mg_coarse_solve<T>(const T*, T*, const TileGeom&, const MgSweepTable&, int, hipStream_t);             \
  template void mgp_smooth<T>(const T*, T*, const T*, const TileGeom&, const MgSweepTable&, GhostSides, PcgScalars*, \
                              double*, unsigned*, hipStream_t);                                                      \
  template void mgp_residual_restrict<T>(const T*, const T*, const TileGeom&, GhostSides, T*, const TileGeom&,       \
                                         Stencil5Coeffs, hipStream_t);                                               \
  template void mgp_prolong_add<T>(const T*, const TileGeom&, T*, const TileGeom&, hipStream_t, GhostSides);          \
  template void mgp_coarse_solve<T>(const T*, T*, const TileGeom&, const MgSweepTable&, int, GhostSides, PcgScalars*, \
                                    hipStream_t);
MXS_MG_INSTANTIATE(float)
MXS_MG_INSTANTIATE(double)
#undef MXS_MG_INSTANTIATE

}  // namespace kernels
}  // namespace mxs
