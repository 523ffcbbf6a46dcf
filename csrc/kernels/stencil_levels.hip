// Level-table passes of the Chebyshev relaxation (mxs/kernels/relaxation.hpp):
// kernels::stencil5_tb_levels and kernels::stencil5_tb_held_levels, the
// contracts of stencil5_tb (no wrap, per-step form) and stencil5_tb_held with
// one coefficient pair per level. The bulk runs on the level-table pipeline
// (stencil_pipe_levels.hpp); the frame along fixed edges, and any rectangle the
// pipeline cannot take, on the held tile of stencil_held.hpp with the table
// indexed by its run-time level loop. Depths: fp32 20 / 24, fp64 12 / 16.
// With a correction tile `corr` (the source term, docs/ARCHITECTURE.md "Source
// term") the same launch ends with out += corr on the rectangle, one rounded
// add per cell ("stream_pipe_levels_src", "held_levels_src"); only the
// rectangle's cells of `corr` are read. Also the build step of that tile:
// source_axpy.
#include <hip/hip_runtime.h>

#include "mxs/core/error.hpp"
#include "mxs/kernels/kernels.hpp"
#include "mxs/runtime/hip_utils.hpp"

#include "stencil_held.hpp"
#include "stencil_pipe_levels.hpp"

namespace mxs {
namespace kernels {
namespace {
using namespace detail;

// The two supported depths of T: fp32 20 / 24, fp64 12 / 16.
template <typename T>
constexpr int level_depth(int i) {
  return sizeof(T) == 4 ? (i == 0 ? 20 : 24) : (i == 0 ? 12 : 16);
}

template <typename T>
void check_levels(const char* who, const TileGeom& g, const LevelTable& t, index_t x0, index_t x1, index_t y0, index_t y1,
                  const T* out, const T* corr) {
  MXS_CHECK(relaxation_depth_supported(int(sizeof(T)), t.n),
            who << ": a level table of " << t.n << " levels has no kernel (fp32: 20 or 24, fp64: 12 or 16)");
  check_block_rect<T>(who, g, t.n, x0, x1, y0, y1);
  MXS_CHECK(corr != out, who << ": the correction tile must not be the output");
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

// The table's doubles rounded to T once, here on the host, into the source a
// kernel takes: one array per coefficient for the held tile, pairs (and the
// correction tile) for the pipeline.
template <typename T, int S>
void launch_held_levels(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                        const LevelTable& t, unsigned hold, const T* corr, hipStream_t s) {
  LevelArray<T, S> c0, c1;
  for (int l = 0; l < S; ++l) {
    c0.v[l] = T(t.center[l]);
    c1.v[l] = T(t.neighbor[l]);
  }
  if (corr == nullptr) launch_held<T, S>(in, out, g, x0, x1, y0, y1, c0, c1, hold, s);
  else launch_held<T, S>(in, out, g, x0, x1, y0, y1, c0, c1, hold, s, corr);
}
template <typename T, int S>
void launch_levels_pipe(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                        const LevelTable& t, const T* corr, hipStream_t s) {
  LevelPairsSrc<T, S> cs;
  for (int l = 0; l < S; ++l) cs.pairs.v[l] = CoeffPair<T>{T(t.center[l]), T(t.neighbor[l])};
  cs.corr = corr;
  if (corr == nullptr) launch_pipe_levels<T, S>(in, out, g, x0, x1, y0, y1, cs.pairs, "stream_pipe_levels", s);
  else launch_pipe_levels<T, S>(in, out, g, x0, x1, y0, y1, cs, "stream_pipe_levels_src", s);
}

// tile core += w * src core, with fixed rounding points: the product is
// rounded, then the sum. The pragma keeps the compiler from contracting the two
// into an fma (HIP's __fmul_rn / __fadd_rn are the plain operators and would be
// contracted too; checked in the -S output: v_mul, then v_add).
template <typename T>
__global__ __launch_bounds__(256) void source_axpy_kernel(T* __restrict__ tile, const T* __restrict__ src, index_t pitch,
                                                          index_t core_off, index_t W, index_t H, T w) {
#pragma clang fp contract(off)
  const index_t x = index_t(blockIdx.x) * 256 + threadIdx.x;
  if (x >= W) return;
  for (index_t y = blockIdx.y; y < H; y += gridDim.y) {
    const index_t at = core_off + y * pitch + x;
    const T p = w * src[at];
    tile[at] = tile[at] + p;
  }
}
}  // namespace

template <typename T>
void stencil5_tb_held_levels(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                             const LevelTable& t, unsigned hold, const T* corr, hipStream_t s) {
  if (x1 <= x0 || y1 <= y0) return;
  check_levels<T>("stencil5_tb_held_levels", g, t, x0, x1, y0, y1, out, corr);
  MXS_CHECK((hold & ~unsigned(kHoldTop | kHoldBottom | kHoldLeft | kHoldRight)) == 0,
            "stencil5_tb_held_levels: hold takes the HoldSide bits only, got " << hold);
  if (t.n == level_depth<T>(0)) launch_held_levels<T, level_depth<T>(0)>(in, out, g, x0, x1, y0, y1, t, hold, corr, s);
  else launch_held_levels<T, level_depth<T>(1)>(in, out, g, x0, x1, y0, y1, t, hold, corr, s);
  note_launch(corr == nullptr ? "held_levels" : "held_levels_src");
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void stencil5_tb_levels(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                        const LevelTable& t, const T* corr, hipStream_t s) {
  if (x1 <= x0 || y1 <= y0) return;
  check_levels<T>("stencil5_tb_levels", g, t, x0, x1, y0, y1, out, corr);
  // Thin rectangles (the thin-strip tiles of launch_tb) and anything else the
  // pipeline cannot take go to the held tile with no side held: the same result.
  if (!levels_pipe_takes<T>(g, t.n, x0, x1, y0, y1))
    return stencil5_tb_held_levels<T>(in, out, g, x0, x1, y0, y1, t, 0u, corr, s);
  if (t.n == level_depth<T>(0)) launch_levels_pipe<T, level_depth<T>(0)>(in, out, g, x0, x1, y0, y1, t, corr, s);
  else launch_levels_pipe<T, level_depth<T>(1)>(in, out, g, x0, x1, y0, y1, t, corr, s);
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void source_axpy(T* tile, const T* src, const TileGeom& g, double w, hipStream_t s) {
  MXS_CHECK(tile != src, "source_axpy: the two tiles must differ");
  if (g.width <= 0 || g.height <= 0) return;
  const dim3 grid(unsigned((g.width + 255) / 256), unsigned(std::min<index_t>(g.height, 1024)));
  source_axpy_kernel<T><<<grid, 256, 0, s>>>(tile, src, g.pitch, g.core_offset(), g.width, g.height, T(w));
  MXS_HIP_CHECK_LAUNCH();
}

#define MXS_INST_LEVELS(T)                                                                                        \
  template void stencil5_tb_levels<T>(const T*, T*, const TileGeom&, index_t, index_t, index_t, index_t,           \
                                      const LevelTable&, const T*, hipStream_t);                                  \
  template void stencil5_tb_held_levels<T>(const T*, T*, const TileGeom&, index_t, index_t, index_t, index_t,      \
                                           const LevelTable&, unsigned, const T*, hipStream_t);                   \
  template void source_axpy<T>(T*, const T*, const TileGeom&, double, hipStream_t);
MXS_INST_LEVELS(float)
MXS_INST_LEVELS(double)
#undef MXS_INST_LEVELS

}  // namespace kernels
}  // namespace mxs
