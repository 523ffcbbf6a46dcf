// Level-table pipeline with a correction tile, fp32 S = 20 and 24: the
// source-term passes (stencil_pipe_levels.hpp, LevelPairsSrc).
#include "stencil_pipe_levels.hpp"

namespace mxs {
namespace kernels {
namespace detail {

template <typename T, int S, typename C>
void launch_pipe_levels(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                        const C& cs, const char* name, hipStream_t s) {
  launch_pipe_levels_impl<T, S, C>(in, out, g, x0, x1, y0, y1, cs, name, s);
}

MXS_INST_PIPE_LEVELS(float, 20, LevelPairsSrc);
MXS_INST_PIPE_LEVELS(float, 24, LevelPairsSrc);

}  // namespace detail
}  // namespace kernels
}  // namespace mxs
