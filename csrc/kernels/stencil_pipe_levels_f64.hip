// Level-table pipeline instantiations, fp64 S = 12 and 16 (wide-lane body,
// per-step form, ghost-ring tiles): the Chebyshev relaxation passes.
#include "stencil_pipe_levels.hpp"

namespace mxs {
namespace kernels {
namespace detail {

template <typename T, int S>
void launch_pipe_levels(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                        const LevelTable& t, hipStream_t s) {
  launch_pipe_levels_impl<T, S>(in, out, g, x0, x1, y0, y1, t, s);
}

template void launch_pipe_levels<double, 12>(const double*, double*, const TileGeom&, index_t, index_t, index_t, index_t,
                                             const LevelTable&, hipStream_t);
template void launch_pipe_levels<double, 16>(const double*, double*, const TileGeom&, index_t, index_t, index_t, index_t,
                                             const LevelTable&, hipStream_t);

}  // namespace detail
}  // namespace kernels
}  // namespace mxs
