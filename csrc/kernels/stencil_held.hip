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
  MXS_CHECK(steps >= 1 && steps <= held_max_steps<T>(),
            "stencil5_tb_held: steps must be in [1, " << held_max_steps<T>() << "], got " << steps);
  check_block_rect<T>("stencil5_tb_held", g, steps, x0, x1, y0, y1);
  MXS_CHECK((hold & ~unsigned(kHoldTop | kHoldBottom | kHoldLeft | kHoldRight)) == 0,
            "stencil5_tb_held: hold takes the HoldSide bits only, got " << hold);
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
