// Host-side checks shared by the level-table passes with and without a
// correction tile (stencil_levels.hip, stencil_levels_src.hip).
#pragma once

#include "mxs/core/error.hpp"
#include "mxs/kernels/kernels.hpp"

#include "stencil_held.hpp"
#include "stencil_pipe.hpp"

namespace mxs {
namespace kernels {
namespace detail {

// The two supported depths of T: fp32 20 / 24, fp64 12 / 16.
template <typename T>
constexpr int level_depth(int i) {
  return sizeof(T) == 4 ? (i == 0 ? 20 : 24) : (i == 0 ? 12 : 16);
}

template <typename T>
void check_levels(const char* who, const TileGeom& g, const LevelTable& t, index_t x0, index_t x1, index_t y0, index_t y1) {
  constexpr int N = Vec16<T>::N;
  const int steps = t.n;
  MXS_CHECK(relaxation_depth_supported(int(sizeof(T)), steps),
            who << ": a level table of " << steps << " levels has no kernel (fp32: 20 or 24, fp64: 12 or 16)");
  MXS_CHECK(x0 >= 0 && y0 >= 0 && x1 <= g.width && y1 <= g.height, who << ": rect out of the core");
  MXS_CHECK(x0 % N == 0, who << ": x0 must be a multiple of the vector width");
  MXS_CHECK((g.pitch % N) == 0 && ((g.x_origin + g.halo_x) % N) == 0, who << " needs a TileGeom::aligned layout");
  const int sa = ((steps + N - 1) / N) * N;
  MXS_CHECK(g.halo_x >= steps && g.halo_y >= steps,
            who << ": ghost ring (" << g.halo_x << ") shallower than the level table (" << steps << ")");
  MXS_CHECK(g.x_origin + g.halo_x >= sa && g.pitch >= g.x_origin + g.halo_x + ((g.width + N - 1) / N) * N + sa,
            who << ": row padding too small for the x apron");
}

// Whether the level-table pipeline takes the rectangle (else the held tile
// with no side held): whole 4-cell lane vectors and rows narrow enough for its
// descriptor-sized pieces; fp64 also needs its apron inside the padding
// (wide_pipe_ok).
template <typename T>
bool levels_pipe_takes(const TileGeom& g, int n, index_t x0, index_t x1, index_t y0, index_t y1) {
  constexpr int NW = sizeof(T) == 4 ? 32 : 16;
  bool pipe = x0 % 4 == 0 && x1 % 4 == 0 && x1 - x0 > NW && y1 - y0 > 16 && chunk_rows_fit(g.pitch, sizeof(T));
  if constexpr (sizeof(T) == 8) {
    if (pipe) pipe = n == 12 ? wide_pipe_ok<T, 12, false>(g, x0, x1) : wide_pipe_ok<T, 16, false>(g, x0, x1);
  }
  return pipe;
}

}  // namespace detail
}  // namespace kernels
}  // namespace mxs
