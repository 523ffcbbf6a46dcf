// S-step Jacobi over a core rectangle beside fixed (non-periodic) edges:
// kernels::stencil5_tb_held. The solver runs the bulk of a tile with physical
// sides on the unchanged stencil5_tb kernels (the interior of
// fixed_edge_split(), which reads no held cell) and only the frame, S cells
// thick along the held sides, here: an LDS tile that recomputes its whole
// staged window at every level and leaves the held cells alone
// (stencil_held.hpp). About 1% of the cells of an 8192^2 tile at S = 20.
#include <hip/hip_runtime.h>

#include "mxs/core/error.hpp"
#include "mxs/kernels/kernels.hpp"
#include "mxs/runtime/hip_utils.hpp"

#include "stencil_held.hpp"

namespace mxs {
namespace kernels {
namespace detail {
// stencil.hip: the last-launch record
void note_launch(const char* kernel, const PipeForm& form = {}, bool split = false, bool block_prio = false);
}

namespace {
using namespace detail;

template <typename T, int S, int TW, int TH>
void launch_held_tile(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1, T c0, T c1,
                      unsigned hold, hipStream_t s) {
  const size_t lds = held_lds_bytes<T, S, TW, TH>();
  const dim3 grid(unsigned((x1 - x0 + TW - 1) / TW), unsigned((y1 - y0 + TH - 1) / TH));
  stencil5_tb_held_kernel<T, S, TW, TH><<<grid, 256, lds, s>>>(in, out, g.pitch, g.core_offset(), g.width, g.height, x0,
                                                              x1, y0, y1, c0, c1, hold);
}

// Tile shape by rectangle shape, as launch_tb does for the overlap schedule's
// thin strips: a column strip (the left / right frame: S columns rounded to
// whole vectors) gets the tall narrow tile, a row strip (the top / bottom
// frame: S rows) the wide flat one, anything else the general tile.
template <typename T, int S>
void launch_held(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1, T c0, T c1,
                 unsigned hold, hipStream_t s) {
  using Sh = HeldShape<T, S>;
  if (x1 - x0 <= Sh::NW + Sh::NW / 4)
    return launch_held_tile<T, S, Sh::NW, Sh::NH>(in, out, g, x0, x1, y0, y1, c0, c1, hold, s);
  if (y1 - y0 <= Sh::FH) return launch_held_tile<T, S, Sh::FW, Sh::FH>(in, out, g, x0, x1, y0, y1, c0, c1, hold, s);
  launch_held_tile<T, S, Sh::GW, Sh::GH>(in, out, g, x0, x1, y0, y1, c0, c1, hold, s);
}

template <typename T>
constexpr int held_max_steps() {
  return sizeof(T) == 4 ? kMaxTimeBlockDeep : kMaxTimeBlock;
}

template <typename T, int S = 1>
void dispatch_held(int steps, const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                   T c0, T c1, unsigned hold, hipStream_t s) {
  if constexpr (S <= held_max_steps<T>()) {
    if (steps == S) return launch_held<T, S>(in, out, g, x0, x1, y0, y1, c0, c1, hold, s);
    return dispatch_held<T, S + 1>(steps, in, out, g, x0, x1, y0, y1, c0, c1, hold, s);
  } else {
    MXS_CHECK(false, "stencil5_tb_held: steps must be in [1, " << held_max_steps<T>() << "], got " << steps);
  }
}
}  // namespace

template <typename T>
void stencil5_tb_held(const T* in, T* out, const TileGeom& g, int steps, index_t x0, index_t x1, index_t y0, index_t y1,
                      Stencil5Coeffs c, unsigned hold, hipStream_t s) {
  if (x1 <= x0 || y1 <= y0) return;
  constexpr int N = Vec16<T>::N;
  MXS_CHECK(steps >= 1 && steps <= held_max_steps<T>(),
            "stencil5_tb_held: steps must be in [1, " << held_max_steps<T>() << "], got " << steps);
  MXS_CHECK(x0 >= 0 && y0 >= 0 && x1 <= g.width && y1 <= g.height, "stencil5_tb_held: rect out of the core");
  MXS_CHECK(x0 % N == 0, "stencil5_tb_held: x0 must be a multiple of the vector width");
  MXS_CHECK((hold & ~unsigned(kHoldTop | kHoldBottom | kHoldLeft | kHoldRight)) == 0,
            "stencil5_tb_held: hold takes the HoldSide bits only, got " << hold);
  MXS_CHECK((g.pitch % N) == 0 && ((g.x_origin + g.halo_x) % N) == 0,
            "stencil5_tb_held needs a TileGeom::aligned layout");
  const int sa = ((steps + N - 1) / N) * N;
  MXS_CHECK(g.halo_x >= steps && g.halo_y >= steps,
            "stencil5_tb_held: ghost ring (" << g.halo_x << ") shallower than the time block (" << steps << ")");
  MXS_CHECK(g.x_origin + g.halo_x >= sa && g.pitch >= g.x_origin + g.halo_x + ((g.width + N - 1) / N) * N + sa,
            "stencil5_tb_held: row padding too small for the x apron");
  dispatch_held<T>(steps, in, out, g, x0, x1, y0, y1, T(c.center), T(c.neighbor), hold, s);
  note_launch("tb_held");
  MXS_HIP_CHECK_LAUNCH();
}

template void stencil5_tb_held<float>(const float*, float*, const TileGeom&, int, index_t, index_t, index_t, index_t,
                                      Stencil5Coeffs, unsigned, hipStream_t);
template void stencil5_tb_held<double>(const double*, double*, const TileGeom&, int, index_t, index_t, index_t, index_t,
                                       Stencil5Coeffs, unsigned, hipStream_t);

}  // namespace kernels
}  // namespace mxs
