// Level-table passes of the Chebyshev relaxation (mxs/kernels/relaxation.hpp):
// kernels::stencil5_tb_levels and kernels::stencil5_tb_held_levels, the
// contracts of stencil5_tb (no wrap, per-step form) and stencil5_tb_held with
// one coefficient pair per level. The bulk runs on the level-table pipeline
// (stencil_pipe_levels.hpp); the frame along fixed edges, and any rectangle the
// pipeline cannot take, on the held tile of stencil_held.hpp with the table
// indexed by its run-time level loop. Depths: fp32 20 / 24, fp64 12 / 16.
#include <hip/hip_runtime.h>

#include "mxs/core/error.hpp"
#include "mxs/kernels/kernels.hpp"
#include "mxs/runtime/hip_utils.hpp"

#include "stencil_levels.hpp"
#include "stencil_pipe_levels.hpp"

namespace mxs {
namespace kernels {
namespace {
using namespace detail;

template <typename T, int S, int TW, int TH>
__global__ __launch_bounds__(256) void stencil5_tb_held_levels_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                                      index_t pitch, index_t core_off, index_t W,
                                                                      index_t H, index_t x_begin, index_t x_end,
                                                                      index_t y_begin, index_t y_end,
                                                                      const LevelArray<T, S> c0, const LevelArray<T, S> c1,
                                                                      unsigned hold) {
  // stencil5_tb_held_kernel (stencil_held.hpp) with the coefficients of level s
  // read from the tables in the kernel arguments; written out again, see the
  // note at the top of stencil_pipe_kernels.hpp.
  constexpr int N = Vec16<T>::N;
  constexpr int SA = ((S + N - 1) / N) * N;
  constexpr int LW = TW + 2 * SA;
  constexpr int LP = LW + 2 * N;
  constexpr int LH = TH + 2 * S;
  constexpr int NV = LW / N;
  constexpr int CELLS = (LH - 2) * NV;      // vectors updated per step
  constexpr int PER = (CELLS + 255) / 256;  // per thread
  static_assert(TW % N == 0, "tile width must be a multiple of the vector width");
  static_assert(held_lds_bytes<T, S, TW, TH>() <= size_t(kHeldLdsBytes), "held tile over its LDS budget");
  using V = typename Vec16<T>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_held_levels[];
  T* buf = reinterpret_cast<T*>(smem_held_levels);

  const index_t tx0 = x_begin + index_t(blockIdx.x) * TW;
  const index_t ty0 = y_begin + index_t(blockIdx.y) * TH;
  const int tid = threadIdx.x;

  // Stage rows [ty0 - S, ty0 + TH + S) x columns [tx0 - SA, tx0 + TW + SA),
  // clipped to the tile's ghost ring (the launcher checks ring and padding).
  for (int i = tid; i < LH * NV; i += 256) {
    const int r = i / NV, v = i - r * NV;
    const index_t gy = ty0 - S + r;
    const index_t gx = tx0 - SA + index_t(v) * N;
    V val = V(T(0));
    if (gy < H + S && gx < W + SA) val = *reinterpret_cast<const V*>(in + core_off + gy * pitch + gx);
    *reinterpret_cast<V*>(buf + r * LP + N + v * N) = val;
  }
  __syncthreads();

  const index_t row0 = index_t(S) - ty0, col0 = index_t(SA) - tx0;
  const bool hold_t = (hold & kHoldTop) != 0, hold_b = (hold & kHoldBottom) != 0;
  const bool hold_l = (hold & kHoldLeft) != 0, hold_r = (hold & kHoldRight) != 0;

#pragma unroll 1
  for (int s = 0; s < S; ++s) {
    const T k0 = c0.v[s], k1 = c1.v[s];  // workgroup-uniform: scalar loads
    V res[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * 256;
      if (i < CELLS) {
        const int r = 1 + i / NV, v = i - (r - 1) * NV;
        const int base = r * LP + N + v * N;
        const V mid = *reinterpret_cast<const V*>(buf + base);
        const index_t gy = index_t(r) - row0, gx = index_t(v) * N - col0;
        int live = N;
        if ((hold_t && gy < 0) || (hold_b && gy >= H) || (hold_l && gx < 0)) live = 0;
        else if (hold_r && gx + N > W) live = gx >= W ? 0 : int(W - gx);
        V o = mid;
        if (live > 0) {
          const V up = *reinterpret_cast<const V*>(buf + base - LP);
          const V dn = *reinterpret_cast<const V*>(buf + base + LP);
          const T left = buf[base - 1];
          const T right = buf[base + N];
          const V n = jac_vec<T, V, N>(up, mid, dn, left, right, k0, k1);
#pragma unroll
          for (int q = 0; q < N; ++q)
            if (q < live) o[q] = n[q];
        }
        res[k] = o;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * 256;
      if (i < CELLS) {
        const int r = 1 + i / NV, v = i - (r - 1) * NV;
        *reinterpret_cast<V*>(buf + r * LP + N + v * N) = res[k];
      }
    }
    __syncthreads();
  }

  constexpr int OV = TW / N;
  for (int i = tid; i < TH * OV; i += 256) {
    const int r = i / OV, v = i - r * OV;
    const index_t gy = ty0 + r, gx = tx0 + index_t(v) * N;
    if (gy >= y_end || gx >= x_end) continue;
    const V o = *reinterpret_cast<const V*>(buf + (r + S) * LP + N + SA + v * N);
    T* p = out + core_off + gy * pitch + gx;
    if (gx + N <= x_end) {
      __builtin_nontemporal_store(o, reinterpret_cast<V*>(p));
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (gx + k < x_end) p[k] = o[k];
    }
  }
}

template <typename T, int S, int TW, int TH>
void launch_held_levels_tile(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                             const LevelTable& t, unsigned hold, hipStream_t s) {
  LevelArray<T, S> c0, c1;
  level_arrays<T, S>(t, &c0, &c1);
  const size_t lds = held_lds_bytes<T, S, TW, TH>();
  const dim3 grid(unsigned((x1 - x0 + TW - 1) / TW), unsigned((y1 - y0 + TH - 1) / TH));
  stencil5_tb_held_levels_kernel<T, S, TW, TH><<<grid, 256, lds, s>>>(in, out, g.pitch, g.core_offset(), g.width,
                                                                     g.height, x0, x1, y0, y1, c0, c1, hold);
}

// Tile shape by rectangle shape, as stencil_held.hip's launch_held.
template <typename T, int S>
void launch_held_levels(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                        const LevelTable& t, unsigned hold, hipStream_t s) {
  using Sh = HeldShape<T, S>;
  if (x1 - x0 <= Sh::NW + Sh::NW / 4)
    return launch_held_levels_tile<T, S, Sh::NW, Sh::NH>(in, out, g, x0, x1, y0, y1, t, hold, s);
  if (y1 - y0 <= Sh::FH) return launch_held_levels_tile<T, S, Sh::FW, Sh::FH>(in, out, g, x0, x1, y0, y1, t, hold, s);
  launch_held_levels_tile<T, S, Sh::GW, Sh::GH>(in, out, g, x0, x1, y0, y1, t, hold, s);
}

}  // namespace

template <typename T>
void stencil5_tb_held_levels(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                             const LevelTable& t, unsigned hold, hipStream_t s) {
  if (x1 <= x0 || y1 <= y0) return;
  check_levels<T>("stencil5_tb_held_levels", g, t, x0, x1, y0, y1);
  MXS_CHECK((hold & ~unsigned(kHoldTop | kHoldBottom | kHoldLeft | kHoldRight)) == 0,
            "stencil5_tb_held_levels: hold takes the HoldSide bits only, got " << hold);
  if (t.n == level_depth<T>(0)) launch_held_levels<T, level_depth<T>(0)>(in, out, g, x0, x1, y0, y1, t, hold, s);
  else launch_held_levels<T, level_depth<T>(1)>(in, out, g, x0, x1, y0, y1, t, hold, s);
  note_launch("held_levels");
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T>
void stencil5_tb_levels(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
                        const LevelTable& t, hipStream_t s) {
  if (x1 <= x0 || y1 <= y0) return;
  check_levels<T>("stencil5_tb_levels", g, t, x0, x1, y0, y1);
  // Thin rectangles (the thin-strip tiles of launch_tb) and anything else the
  // pipeline cannot take go to the held tile with no side held: the same result.
  const bool pipe = levels_pipe_takes<T>(g, t.n, x0, x1, y0, y1);
  if (!pipe) return stencil5_tb_held_levels<T>(in, out, g, x0, x1, y0, y1, t, 0u, s);
  if (t.n == level_depth<T>(0)) launch_pipe_levels<T, level_depth<T>(0)>(in, out, g, x0, x1, y0, y1, t, s);
  else launch_pipe_levels<T, level_depth<T>(1)>(in, out, g, x0, x1, y0, y1, t, s);
  MXS_HIP_CHECK_LAUNCH();
}

#define MXS_INST_LEVELS(T)                                                                                          \
  template void stencil5_tb_levels<T>(const T*, T*, const TileGeom&, index_t, index_t, index_t, index_t,             \
                                      const LevelTable&, hipStream_t);                                              \
  template void stencil5_tb_held_levels<T>(const T*, T*, const TileGeom&, index_t, index_t, index_t, index_t,        \
                                           const LevelTable&, unsigned, hipStream_t);
MXS_INST_LEVELS(float)
MXS_INST_LEVELS(double)
#undef MXS_INST_LEVELS

}  // namespace kernels
}  // namespace mxs
