// The single-buffer LDS tile of the time-blocked passes, and the LDS sizes of both tile forms.
#pragma once

#include "stencil_bodies.hpp"

namespace mxs::kernels::detail {

// LDS bytes of the ping-pong LDS tile (bench/tune_kernels.hpp: stencil5_tb_kernel,
// the tuner's alternative); the single-buffer tile below takes half.
template <typename T, int S, int TW, int TH>
constexpr size_t tb_lds_bytes() {
  constexpr int N = Vec16<T>::N;
  constexpr int SA = ((S + N - 1) / N) * N;
  return size_t(2) * (TH + 2 * S) * (TW + 2 * SA + 2 * N) * sizeof(T);
}

// Single-LDS-buffer variant of stencil5_tb_kernel: each step reads its cells into
// registers (a compile-time number of vectors per thread, statically indexed so
// they stay in VGPRs), barrier, writes them back in place, barrier. Half the LDS
// of the ping-pong form, so more workgroups per CU keep HBM busy while others
// compute.
template <typename T, int S, int TW, int TH, bool WRAP>
__global__ __launch_bounds__(256) void stencil5_tb1_kernel(const T* __restrict__ in, T* __restrict__ out, index_t pitch,
                                                          index_t core_off, index_t W, index_t H, index_t x_begin,
                                                          index_t x_end, index_t y_begin, index_t y_end, T c0, T c1) {
  constexpr int N = Vec16<T>::N;
  constexpr int SA = ((S + N - 1) / N) * N;
  constexpr int LW = TW + 2 * SA;
  constexpr int LP = LW + 2 * N;
  constexpr int LH = TH + 2 * S;
  constexpr int NV = LW / N;
  constexpr int CELLS = (LH - 2) * NV;            // vectors updated per step
  constexpr int PER = (CELLS + 255) / 256;        // per thread
  static_assert(TW % N == 0, "tile width must be a multiple of the vector width");
  using V = typename Vec16<T>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_tb1[];
  T* buf = reinterpret_cast<T*>(smem_tb1);

  const index_t tx0 = x_begin + index_t(blockIdx.x) * TW;
  const index_t ty0 = y_begin + index_t(blockIdx.y) * TH;
  const int tid = threadIdx.x;
  // Staged coordinates stay within one period of the tile unless the tile is
  // smaller than the workgroup's footprint: then fall back to a full modulo.
  const bool one_period = W >= TW + 2 * SA && H >= TH + 2 * S;

  for (int i = tid; i < LH * NV; i += 256) {
    const int r = i / NV, v = i - r * NV;
    index_t gy = ty0 - S + r;
    index_t gx = tx0 - SA + index_t(v) * N;
    V val = V(T(0));
    bool ok;
    if constexpr (WRAP) {
      if (one_period) {
        gy = gy < 0 ? gy + H : (gy >= H ? gy - H : gy);
        gx = gx < 0 ? gx + W : (gx >= W ? gx - W : gx);
      } else {
        gy = ((gy % H) + H) % H;
        gx = ((gx % W) + W) % W;
      }
      ok = true;
    } else {
      ok = gy < H + S && gx < W + SA;
    }
    if (ok) val = *reinterpret_cast<const V*>(in + core_off + gy * pitch + gx);
    *reinterpret_cast<V*>(buf + r * LP + N + v * N) = val;
  }
  __syncthreads();

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
        const V up = *reinterpret_cast<const V*>(buf + base - LP);
        const V dn = *reinterpret_cast<const V*>(buf + base + LP);
        const T left = buf[base - 1];
        const T right = buf[base + N];
        res[k] = jac_vec<T, V, N>(up, mid, dn, left, right, c0, c1);
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
constexpr size_t tb1_lds_bytes() {
  return tb_lds_bytes<T, S, TW, TH>() / 2;
}

}  // namespace mxs::kernels::detail
