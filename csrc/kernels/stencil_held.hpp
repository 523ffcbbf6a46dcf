// Device code of the held-side S-step tile (kernels::stencil5_tb_held): the
// single-buffer LDS tile of stencil_tile.hpp (stencil5_tb1_kernel) with fixed
// boundary values. Like that kernel it stages the tile plus an S-deep apron and
// updates EVERY staged cell in place at each of the S levels (no shrinking
// trapezoid), so holding a physical edge only means not writing some cells
// back: a cell outside the core on a held side keeps its staged input value at
// every level.
//   * held rows (above row 0 / from row H on): whole LDS rows;
//   * held columns left of column 0: whole vectors (the core starts on a
//     vector boundary and so does every staged vector);
//   * held columns from column W on: per element, for a width that is not a
//     whole number of vectors.
// Per-step form only (the jac<T> fma sequence of every other kernel).
//
// One body for every coefficient source (stencil_bodies.hpp: level_coeff): C is
// T, the uniform pair of stencil5_tb_held, or LevelArray<T, S>, a level table
// indexed by the run-time level loop (stencil5_tb_held_levels). CORR is an
// empty pack, or T: then `corr`, a tile of the pass's geometry, is added to
// every cell of the write-out (the source term). How the two are spelled
// matters to the generated code: see the note at the top of
// stencil_pipe_kernels.hpp.
// Also the host side all entries share: the tile launcher, the shape chooser
// and the rectangle check of an S-step block.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "mxs/core/error.hpp"
#include "mxs/kernels/kernels.hpp"
#include "stencil_bodies.hpp"
#include "stencil_tile.hpp"

namespace mxs {
namespace kernels {
namespace detail {

// LDS budget of one held tile: the largest tile stencil5_tb1_kernel runs today
// (tb1_lds_bytes<float, 16, 32, 128>), so three workgroups share a CU's 160 KB.
constexpr int kHeldLdsBytes = 46080;

template <typename T, int S, int TW, int TH>
constexpr size_t held_lds_bytes() {
  return tb1_lds_bytes<T, S, TW, TH>();
}

template <typename T, int S, int TW, int TH, typename C, typename... CORR>
__global__ __launch_bounds__(256) void stencil5_tb_held_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                               const CORR* __restrict__... corr, index_t pitch,
                                                               index_t core_off, index_t W, index_t H, index_t x_begin,
                                                               index_t x_end, index_t y_begin, index_t y_end, const C c0,
                                                               const C c1, unsigned hold) {
  static_assert(sizeof...(CORR) <= 1 && (std::is_same<CORR, T>::value && ...),
                "at most one correction tile, of the element type");
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
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_held[];
  T* buf = reinterpret_cast<T*>(smem_held);

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

  // Staged coordinates of the core's edges: LDS row r is core row r - row0,
  // staged vector v starts at core column v * N - col0.
  const index_t row0 = index_t(S) - ty0, col0 = index_t(SA) - tx0;
  const bool hold_t = (hold & kHoldTop) != 0, hold_b = (hold & kHoldBottom) != 0;
  const bool hold_l = (hold & kHoldLeft) != 0, hold_r = (hold & kHoldRight) != 0;

#pragma unroll 1
  for (int s = 0; s < S; ++s) {
    const T k0 = level_coeff(c0, s), k1 = level_coeff(c1, s);  // workgroup-uniform: scalars
    V res[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * 256;
      if (i < CELLS) {
        const int r = 1 + i / NV, v = i - (r - 1) * NV;
        const int base = r * LP + N + v * N;
        const V mid = *reinterpret_cast<const V*>(buf + base);
        const index_t gy = index_t(r) - row0, gx = index_t(v) * N - col0;
        // Elements of this vector that advance: none in a held row or left of
        // a held column 0, those below column W beside a held right side.
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

  // Write-out: the rectangle's cells, plus their correction if there is one, per
  // vector and per element in the ragged tail (x_end <= W, so every cell read
  // from corr is a core cell).
  constexpr int OV = TW / N;
  for (int i = tid; i < TH * OV; i += 256) {
    const int r = i / OV, v = i - r * OV;
    const index_t gy = ty0 + r, gx = tx0 + index_t(v) * N;
    if (gy >= y_end || gx >= x_end) continue;
    const V o = *reinterpret_cast<const V*>(buf + (r + S) * LP + N + SA + v * N);
    const index_t at = core_off + gy * pitch + gx;
    T* p = out + at;
    if constexpr (sizeof...(CORR) == 0) {
      if (gx + N <= x_end) {
        __builtin_nontemporal_store(o, reinterpret_cast<V*>(p));
      } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
          if (gx + k < x_end) p[k] = o[k];
      }
    } else {
      const T* q = (corr, ...) + at;
      if (gx + N <= x_end) {
        const V c = __builtin_nontemporal_load(reinterpret_cast<const V*>(q));
        __builtin_nontemporal_store(o + c, reinterpret_cast<V*>(p));
      } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
          if (gx + k < x_end) p[k] = o[k] + q[k];
      }
    }
  }
}

// Tile shapes per depth, each the largest that fits kHeldLdsBytes:
//   narrow  (column strips, about S columns wide): NW columns x up to 128 rows;
//   flat    (row strips, about S rows tall): max(S, 8) rows x up to 256 columns;
//   general (whatever is left, e.g. a whole small core): GW columns wide.
template <typename T, int S>
struct HeldShape {
  static constexpr int N = Vec16<T>::N;
  static constexpr int SA = ((S + N - 1) / N) * N;
  static constexpr int B = int(sizeof(T));
  static constexpr int row_bytes(int tw) { return (tw + 2 * SA + 2 * N) * B; }
  static constexpr int rows_for(int tw) { return kHeldLdsBytes / row_bytes(tw) - 2 * S; }
  static constexpr int floor8(int x) { return x / 8 * 8; }
  static constexpr int clamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

  static constexpr int NW = sizeof(T) == 4 ? 32 : 16;
  static constexpr int NH = clamp(floor8(rows_for(NW)), 8, 128);
  static constexpr int FH = S < 8 ? 8 : S;
  static constexpr int FW = clamp(floor8(kHeldLdsBytes / (FH + 2 * S) / B - 2 * SA - 2 * N), 8, 256);
  static constexpr int GW = sizeof(T) == 4 ? 64 : 32;
  static constexpr int GH = clamp(floor8(rows_for(GW)), 8, 128);
};

// ------------------------------------------------------------------ host side
template <typename T, int S, int TW, int TH, typename C, typename... CORR>
void launch_held_tile(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1, const C& c0,
                      const C& c1, unsigned hold, hipStream_t s, const CORR*... corr) {
  const size_t lds = held_lds_bytes<T, S, TW, TH>();
  const dim3 grid(unsigned((x1 - x0 + TW - 1) / TW), unsigned((y1 - y0 + TH - 1) / TH));
  stencil5_tb_held_kernel<T, S, TW, TH, C, CORR...><<<grid, 256, lds, s>>>(
      in, out, corr..., g.pitch, g.core_offset(), g.width, g.height, x0, x1, y0, y1, c0, c1, hold);
}

// Tile shape by rectangle shape, as launch_tb does for the overlap schedule's
// thin strips: a column strip (the left / right frame: S columns rounded to
// whole vectors) gets the tall narrow tile, a row strip (the top / bottom
// frame: S rows) the wide flat one, anything else the general tile. `corr`: no
// argument, or the correction tile.
template <typename T, int S, typename C, typename... CORR>
void launch_held(const T* in, T* out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1, const C& c0,
                 const C& c1, unsigned hold, hipStream_t s, const CORR*... corr) {
  using Sh = HeldShape<T, S>;
  if (x1 - x0 <= Sh::NW + Sh::NW / 4)
    return launch_held_tile<T, S, Sh::NW, Sh::NH>(in, out, g, x0, x1, y0, y1, c0, c1, hold, s, corr...);
  if (y1 - y0 <= Sh::FH) return launch_held_tile<T, S, Sh::FW, Sh::FH>(in, out, g, x0, x1, y0, y1, c0, c1, hold, s, corr...);
  launch_held_tile<T, S, Sh::GW, Sh::GH>(in, out, g, x0, x1, y0, y1, c0, c1, hold, s, corr...);
}

// What every `steps`-level block over [x0, x1) x [y0, y1) of a tile needs:
// the rectangle inside the core with x0 on a vector boundary, the aligned
// layout and, where the block reads a ghost ring (`ring`: every pass but the
// wrapping stencil5_tb), a ring of `steps` cells and row padding for the x
// apron, `steps` rounded up to whole vectors.
template <typename T>
void check_block_rect(const char* who, const TileGeom& g, int steps, index_t x0, index_t x1, index_t y0, index_t y1,
                      bool ring = true) {
  constexpr int N = Vec16<T>::N;
  MXS_CHECK(x0 >= 0 && y0 >= 0 && x1 <= g.width && y1 <= g.height, who << ": rect out of the core");
  MXS_CHECK(x0 % N == 0, who << ": x0 must be a multiple of the vector width");
  MXS_CHECK((g.pitch % N) == 0 && ((g.x_origin + g.halo_x) % N) == 0, who << " needs a TileGeom::aligned layout");
  if (!ring) return;
  const int sa = ((steps + N - 1) / N) * N;
  MXS_CHECK(g.halo_x >= steps && g.halo_y >= steps,
            who << ": ghost ring (" << g.halo_x << ") shallower than the time block (" << steps << ")");
  MXS_CHECK(g.x_origin + g.halo_x >= sa && g.pitch >= g.x_origin + g.halo_x + ((g.width + N - 1) / N) * N + sa,
            who << ": row padding too small for the x apron");
}

}  // namespace detail
}  // namespace kernels
}  // namespace mxs
