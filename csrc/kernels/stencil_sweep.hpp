// One-step kernels: the register-roll sweep, the LDS tile, the scalar rectangle, the box stencil.
#pragma once

#include "stencil_bodies.hpp"

namespace mxs::kernels::detail {

// ------------------------------------------------------------- RegisterRoll
// WX waves side by side along x (4/WX stacked along y) per 256-thread workgroup;
// NT = non-temporal (streaming) stores, NTL = non-temporal loads.
// WRAP: periodic wrap-around addressing inside the tile (rows -1 / H map to H-1 / 0,
// columns -1 / W to W-1 / 0) — the fused self-exchange of a 1x1 periodic grid, so
// no ghost cell is read or written. Requires W % VEC == 0.
template <typename T, int ROWS, int CH, bool NT, int WX = 1, bool NTL = false, int NW = kWavesPerBlock,
          bool WRAP = false>
__global__ __launch_bounds__(NW * kWaveSize) void stencil5_roll_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                               index_t pitch, index_t core_off, index_t W,
                                                               index_t row_begin, index_t row_end, T c0, T c1,
                                                               index_t H = 0) {
  static_assert(ROWS % CH == 0, "ROWS must be a multiple of CH");
  constexpr int N = Vec16<T>::N;
  constexpr int SEG = kWaveSize * N;
  using V = typename Vec16<T>::type;

  const int lane = threadIdx.x & (kWaveSize - 1);
  const int wave = threadIdx.x / kWaveSize;
  constexpr int WY = NW / WX;
  static_assert(NW % WX == 0, "WX must divide the waves per workgroup");
  const int wx = wave % WX, wy = wave / WX;
  const index_t seg_base = (index_t(blockIdx.x) * WX + wx) * SEG;
  const index_t x = seg_base + index_t(lane) * N;
  const index_t y0 = row_begin + (index_t(blockIdx.y) * WY + wy) * ROWS;
  if (y0 >= row_end) return;  // wave-uniform exit
  const index_t y1 = y0 + ROWS < row_end ? y0 + ROWS : row_end;

  const bool load_ok = x < W + N;  // covers the lane right after the last core vector
  const bool active = x < W;
  // Lane whose x+1 neighbour of its last element is not in the next lane's vector:
  // lane 63 (next segment), or under WRAP the lane holding column W-1.
  const bool right_lane = (lane == kWaveSize - 1) || (WRAP && x + N == W);
  const bool right_load = WRAP ? right_lane && active : (lane == kWaveSize - 1) && (seg_base + SEG <= W);
  // Column offsets (relative to x) of the two edge values.
  const index_t left_col = (WRAP && x == 0) ? W - 1 : -1;
  const index_t right_col = (WRAP && x + N == W) ? -x : N;
  const T* __restrict__ pin = in + core_off + x;
  T* __restrict__ pout = out + core_off + x;

  auto row = [&](index_t y) -> index_t {
    if constexpr (WRAP) return y < 0 ? y + H : (y >= H ? y - H : y);
    else return y;
  };
  auto ldv = [&](index_t y) -> V {
    V v = V(T(0));
    const index_t r = row(y);
    if (load_ok) {
      if constexpr (NTL) v = __builtin_nontemporal_load(reinterpret_cast<const V*>(pin + r * pitch));
      else v = *reinterpret_cast<const V*>(pin + r * pitch);
    }
    return v;
  };
  struct Edge {
    T l, r;
  };
  auto lde = [&](index_t y) -> Edge {
    Edge e{T(0), T(0)};
    const index_t r = row(y);
    if (lane == 0) e.l = pin[r * pitch + left_col];
    if (right_load) e.r = pin[r * pitch + right_col];
    return e;
  };
  auto emit = [&](index_t y, const V& up, const V& mid, const V& dn, Edge emid) {
    T left = __shfl_up(mid[N - 1], 1);
    T right = __shfl_down(mid[0], 1);
    if (lane == 0) left = emid.l;
    if (right_lane) right = emid.r;
    const V o = jac_vec<T, V, N>(up, mid, dn, left, right, c0, c1);
    if (active) {
      T* p = pout + y * pitch;
      if (x + N <= W) {
        if constexpr (NT) __builtin_nontemporal_store(o, reinterpret_cast<V*>(p));
        else *reinterpret_cast<V*>(p) = o;
      } else {
#pragma unroll
        for (int i = 0; i < N; ++i)
          if (x + i < W) p[i] = o[i];
      }
    }
  };

  V up = ldv(y0 - 1);
  V mid = ldv(y0);
  Edge emid = lde(y0);

  if (y1 - y0 == ROWS) {
    // Full strip: chunks of CH rows, loads of a chunk issued before its math.
#pragma unroll 1
    for (int c = 0; c < ROWS; c += CH) {
      V dn[CH];
      Edge edn[CH];
#pragma unroll
      for (int k = 0; k < CH; ++k) {
        dn[k] = ldv(y0 + c + k + 1);
        edn[k] = lde(y0 + c + k + 1);
      }
#pragma unroll
      for (int k = 0; k < CH; ++k) {
        emit(y0 + c + k, up, mid, dn[k], emid);
        up = mid;
        mid = dn[k];
        emid = edn[k];
      }
    }
  } else {
#pragma unroll 1
    for (index_t y = y0; y < y1; ++y) {
      const V dn = ldv(y + 1);
      const Edge edn = lde(y + 1);
      emit(y, up, mid, dn, emid);
      up = mid;
      mid = dn;
      emid = edn;
    }
  }
}

// ----------------------------------------------------------------- LdsTile
// Workgroup tile: TW = 64*N columns x TH rows of outputs, 256 threads.
template <typename T, int TH>
__global__ __launch_bounds__(kBlock) void stencil5_lds_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                              index_t pitch, index_t core_off, index_t W,
                                                              index_t row_begin, index_t row_end, T c0, T c1) {
  constexpr int N = Vec16<T>::N;
  constexpr int TW = kWaveSize * N;
  constexpr int LW = TW + 2 * N;  // staged row: one extra vector on each side (keeps 16 B alignment)
  using V = typename Vec16<T>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);  // (TH + 2) x LW

  const index_t x0 = index_t(blockIdx.x) * TW;
  const index_t y0 = row_begin + index_t(blockIdx.y) * TH;
  const index_t rows = (y0 + TH <= row_end) ? TH : (row_end - y0);
  const int nvec = LW / N;  // vectors per staged row
  // Stage rows y0-1 .. y0+rows (inclusive), columns x0-N .. x0+TW+N-1.
  for (int i = threadIdx.x; i < (rows + 2) * nvec; i += kBlock) {
    const int r = i / nvec, v = i - r * nvec;
    const index_t gx = x0 - N + index_t(v) * N;
    V val = V(T(0));
    if (gx < W + N) val = *reinterpret_cast<const V*>(in + core_off + (y0 - 1 + r) * pitch + gx);
    *reinterpret_cast<V*>(tile + r * LW + v * N) = val;
  }
  __syncthreads();
  // Each thread: one column group of N, rows strided by 4 (one wave per row).
  const int lane = threadIdx.x & (kWaveSize - 1);
  const int wave = threadIdx.x / kWaveSize;
  const index_t x = x0 + index_t(lane) * N;
  if (x >= W) return;
  for (int r = wave; r < rows; r += kWavesPerBlock) {
    const T* up = tile + r * LW + N + lane * N;
    const T* mid = up + LW;
    const T* dn = mid + LW;
    V o;
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = jac<T>(mid[i], up[i], dn[i], mid[i - 1], mid[i + 1], c0, c1);
    T* p = out + core_off + (y0 + r) * pitch + x;
    if (x + N <= W) {
      *reinterpret_cast<V*>(p) = o;
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i)
        if (x + i < W) p[i] = o[i];
    }
  }
}

// ------------------------------------------------------------------ rect
template <typename T>
__global__ __launch_bounds__(kBlock) void stencil5_rect_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                               index_t pitch, index_t core_off, index_t x0,
                                                               index_t w, index_t y0, index_t h, T c0, T c1) {
  const index_t n = w * h;
  const index_t stride = index_t(gridDim.x) * blockDim.x;
  for (index_t i = index_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
    const index_t yy = i / w, xx = i - yy * w;
    const index_t o = core_off + (y0 + yy) * pitch + (x0 + xx);
    out[o] = jac<T>(in[o], in[o - pitch], in[o + pitch], in[o - 1], in[o + 1], c0, c1);
  }
}

// -------------------------------------------------------------- box (LDS)
// Output tile 64 x 16 per 256-thread workgroup: thread (tx, ty) computes column
// tx, rows 4*ty .. 4*ty+3. The (16+2R) x (64+2R) input tile is staged in LDS once;
// every output then reads its (2R+1)^2 taps from LDS, rolling down the 4 rows.
template <typename T, int R>
__global__ __launch_bounds__(kBlock) void stencil_box_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                             index_t pitch, index_t core_off, index_t x0,
                                                             index_t w, index_t y0, index_t h, BoxWeights bw) {
  constexpr int TW = 64, TH = 16, LW = TW + 2 * R + 1;  // +1 breaks the power-of-two row stride
  constexpr int LH = TH + 2 * R, K = 2 * R + 1;
  __shared__ T tile[LH * LW];
  const index_t bx = x0 + index_t(blockIdx.x) * TW;
  const index_t by = y0 + index_t(blockIdx.y) * TH;
  for (int i = threadIdx.x; i < LH * (TW + 2 * R); i += kBlock) {
    const int r = i / (TW + 2 * R), c = i - r * (TW + 2 * R);
    const index_t gx = bx - R + c, gy = by - R + r;
    // Cells past the rectangle are never written; clamp reads to the tile + ghost ring.
    T v = T(0);
    if (gx < x0 + w + R && gy < y0 + h + R) v = in[core_off + gy * pitch + gx];
    tile[r * LW + c] = v;
  }
  __syncthreads();
  float wk[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) wk[i] = bw.w[i];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const index_t gx = bx + tx;
  if (gx >= x0 + w) return;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int r = ty * 4 + rr;
    const index_t gy = by + r;
    if (gy >= y0 + h) break;
    T acc = T(0);
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
#pragma unroll
      for (int kx = 0; kx < K; ++kx) acc = fma_t<T>(T(wk[ky * K + kx]), tile[(r + ky) * LW + tx + kx], acc);
    out[core_off + gy * pitch + gx] = acc;
  }
}

}  // namespace mxs::kernels::detail
