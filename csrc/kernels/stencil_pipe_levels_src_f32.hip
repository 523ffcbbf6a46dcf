// Level-table pipeline with a correction tile, fp32 S = 20 and 24: the
// source-term passes (stencil_pipe_levels_src.hpp).
#include "stencil_pipe_levels_src.hpp"

namespace mxs {
namespace kernels {
namespace detail {

template <typename T, int S>
void launch_pipe_levels_src(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                            const LevelTable& t, const T* corr, hipStream_t s) {
  launch_pipe_levels_src_impl<T, S>(in, out, g, x0, x1, y0, y1, t, corr, s);
}

template void launch_pipe_levels_src<float, 20>(const float*, float*, const TileGeom&, index_t, index_t, index_t,
                                                index_t, const LevelTable&, const float*, hipStream_t);
template void launch_pipe_levels_src<float, 24>(const float*, float*, const TileGeom&, index_t, index_t, index_t,
                                                index_t, const LevelTable&, const float*, hipStream_t);

}  // namespace detail
}  // namespace kernels
}  // namespace mxs
