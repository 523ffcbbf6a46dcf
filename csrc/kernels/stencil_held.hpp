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
#pragma once

#include <hip/hip_runtime.h>

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

template <typename T, int S, int TW, int TH>
__global__ __launch_bounds__(256) void stencil5_tb_held_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                               index_t pitch, index_t core_off, index_t W, index_t H,
                                                               index_t x_begin, index_t x_end, index_t y_begin,
                                                               index_t y_end, T c0, T c1, unsigned hold) {
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
          const V n = jac_vec<T, V, N>(up, mid, dn, left, right, c0, c1);
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

}  // namespace detail
}  // namespace kernels
}  // namespace mxs
