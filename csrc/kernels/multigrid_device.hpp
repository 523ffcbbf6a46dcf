// Device code of the multigrid kernels (kernels.hpp / multigrid.hip): the fused
// source-aware smoother, residual + full weighting, bilinear prolongation and
// the one-workgroup coarse solve. Plain launches: no cross-workgroup waits, no
// spin loops, no inline assembly.
//
// Every expression below is a rounding contract with ops/multigrid.py:
//   sweep        x' = fma(nb, (n + s) + (w + e), ce * c); x' = x' + T(w) * g
//                (the product rounded, then the sum);
//   residual     r = (fma(c1, (n + s) + (w + e), c0 * v) + g) - v;
//   restriction  g_c = (r_c + 0.5 ((rn + rs) + (rw + re))) + 0.25 ((rnw + rne) + (rsw + rse));
//   prolongation see mg_prolong_add_kernel.
// The pragma keeps the compiler from contracting a product and a sum into an
// fma anywhere in this file; the fmas that are meant are written as builtins.
#pragma once

#include <hip/hip_runtime.h>

#include "mxs/kernels/kernels.hpp"

#pragma clang fp contract(off)

namespace mxs {
namespace kernels {
namespace detail {

template <typename T>
__device__ __forceinline__ T mg_fma(T a, T b, T c) {
  if constexpr (sizeof(T) == 8) return __builtin_fma(a, b, c);
  else return __builtin_fmaf(a, b, c);
}

// The sweep table of one launch, in the kernel arguments (a captured launch
// replays the same table): rounded to T once on the host.
template <typename T, int N>
struct MgSweeps {
  T center[N];
  T neighbor[N];
  T weight[N];
};

template <typename T>
__device__ __forceinline__ T mg_sweep(T c, T n, T s, T w, T e, T g, T ce, T nb, T wt) {
  const T x = mg_fma<T>(nb, (n + s) + (w + e), ce * c);
  const T p = wt * g;
  return x + p;
}

// ------------------------------------------------------------------ smoother
// NU sweeps in one launch. A workgroup stages its kMgTw x kMgTh output tile plus
// an NU-deep apron, clipped at the depth-1 ring (cells beyond the ring stage 0
// and are never read by a cell that reaches the output), and advances the
// staged core cells in place: sweep s updates the cells at least s + 1 away
// from the staged window's edge (a shrinking window: what the output tile
// needs). Ring cells are held: they keep their staged value at every sweep.
// g is read on core cells only, once, into registers (a thread owns the same
// cells at every sweep).
constexpr int kMgTw = 64, kMgTh = 32, kMgBlock = 256;

template <typename T, int NU>
__global__ __launch_bounds__(kMgBlock) void mg_smooth_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                             const T* __restrict__ gsrc, index_t pitch,
                                                             index_t core_off, index_t W, index_t H,
                                                             MgSweeps<T, NU> tab) {
  constexpr int LW = kMgTw + 2 * NU, LH = kMgTh + 2 * NU;
  constexpr int LP = LW + 1;  // odd row pitch: column walks spread over the banks
  constexpr int IW = LW - 2, IH = LH - 2;  // cells that can advance (all but the staged edge)
  constexpr int CELLS = IW * IH;
  constexpr int PER = (CELLS + kMgBlock - 1) / kMgBlock;
  __shared__ T buf[LH * LP];

  const index_t tx0 = index_t(blockIdx.x) * kMgTw, ty0 = index_t(blockIdx.y) * kMgTh;
  const int tid = threadIdx.x;

  for (int i = tid; i < LH * LW; i += kMgBlock) {
    const int r = i / LW, c = i - r * LW;
    const index_t gy = ty0 - NU + r, gx = tx0 - NU + c;
    T v = T(0);
    if (gy >= -1 && gy <= H && gx >= -1 && gx <= W) v = in[core_off + gy * pitch + gx];
    buf[r * LP + c] = v;
  }

  // This thread's cells: staged (r, c), whether it is a core cell, its source.
  T gv[PER];
  bool live[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = tid + k * kMgBlock;
    gv[k] = T(0);
    live[k] = false;
    if (i < CELLS) {
      const int r = 1 + i / IW, c = 1 + (i - (i / IW) * IW);
      const index_t gy = ty0 - NU + r, gx = tx0 - NU + c;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        live[k] = true;
        gv[k] = gsrc[core_off + gy * pitch + gx];
      }
    }
  }
  __syncthreads();

#pragma unroll
  for (int s = 0; s < NU; ++s) {
    T res[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * kMgBlock;
      res[k] = T(0);
      if (i < CELLS && live[k]) {
        const int r = 1 + i / IW, c = 1 + (i - (i / IW) * IW);
        if (r > s && r < LH - 1 - s && c > s && c < LW - 1 - s) {
          const int b = r * LP + c;
          res[k] = mg_sweep<T>(buf[b], buf[b - LP], buf[b + LP], buf[b - 1], buf[b + 1], gv[k], tab.center[s],
                               tab.neighbor[s], tab.weight[s]);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * kMgBlock;
      if (i < CELLS && live[k]) {
        const int r = 1 + i / IW, c = 1 + (i - (i / IW) * IW);
        if (r > s && r < LH - 1 - s && c > s && c < LW - 1 - s) buf[r * LP + c] = res[k];
      }
    }
    __syncthreads();
  }

  for (int i = tid; i < kMgTh * kMgTw; i += kMgBlock) {
    const int r = i / kMgTw, c = i - r * kMgTw;
    const index_t gy = ty0 + r, gx = tx0 + c;
    if (gy < H && gx < W) out[core_off + gy * pitch + gx] = buf[(r + NU) * LP + c + NU];
  }
}

// ------------------------------------------------- residual + full weighting
// A workgroup owns kMgCw x kMgCh coarse cells: it stages the fine u window
// (2 kMgCw + 3) x (2 kMgCh + 3) they reach, forms the fine residual of the
// (2 kMgCw + 1) x (2 kMgCh + 1) core cells in LDS (g read once per cell) and
// writes the weighted sums. No fine residual array leaves the workgroup.
// Fine (W, H) odd, coarse ((W - 1) / 2, (H - 1) / 2): all nine fine cells of a
// coarse cell are core cells.
constexpr int kMgCw = 32, kMgCh = 16;

template <typename T>
__global__ __launch_bounds__(kMgBlock) void mg_residual_restrict_kernel(const T* __restrict__ u,
                                                                        const T* __restrict__ gsrc, index_t pitch,
                                                                        index_t core_off, index_t W, index_t H,
                                                                        T* __restrict__ gc, index_t cpitch,
                                                                        index_t ccore_off, index_t CW, index_t CH, T c0,
                                                                        T c1) {
  constexpr int RW = 2 * kMgCw + 1, RH = 2 * kMgCh + 1;  // fine residual cells
  constexpr int UW = RW + 2, UH = RH + 2;                // fine u cells staged
  constexpr int UP = UW, RP = RW;                        // both odd
  __shared__ T ub[UH * UP];
  __shared__ T rb[RH * RP];

  const index_t cx0 = index_t(blockIdx.x) * kMgCw, cy0 = index_t(blockIdx.y) * kMgCh;
  const index_t fx0 = 2 * cx0, fy0 = 2 * cy0;  // first fine residual cell
  const int tid = threadIdx.x;

  for (int i = tid; i < UH * UW; i += kMgBlock) {
    const int r = i / UW, c = i - r * UW;
    const index_t gy = fy0 - 1 + r, gx = fx0 - 1 + c;
    T v = T(0);
    if (gy <= H && gx <= W) v = u[core_off + gy * pitch + gx];  // gy, gx >= -1 always
    ub[r * UP + c] = v;
  }
  __syncthreads();
  for (int i = tid; i < RH * RW; i += kMgBlock) {
    const int r = i / RW, c = i - r * RW;
    const index_t gy = fy0 + r, gx = fx0 + c;
    T res = T(0);
    if (gy < H && gx < W) {
      const int b = (r + 1) * UP + c + 1;
      const T v = ub[b];
      const T a = mg_fma<T>(c1, (ub[b - UP] + ub[b + UP]) + (ub[b - 1] + ub[b + 1]), c0 * v);
      res = (a + gsrc[core_off + gy * pitch + gx]) - v;
    }
    rb[r * RP + c] = res;
  }
  __syncthreads();
  for (int i = tid; i < kMgCh * kMgCw; i += kMgBlock) {
    const int r = i / kMgCw, c = i - r * kMgCw;
    const index_t cy = cy0 + r, cx = cx0 + c;
    if (cy >= CH || cx >= CW) continue;
    const int b = (2 * r + 1) * RP + 2 * c + 1;
    const T edge = (rb[b - RP] + rb[b + RP]) + (rb[b - 1] + rb[b + 1]);
    const T corner = (rb[b - RP - 1] + rb[b - RP + 1]) + (rb[b + RP - 1] + rb[b + RP + 1]);
    gc[ccore_off + cy * cpitch + cx] = (rb[b] + T(0.5) * edge) + T(0.25) * corner;
  }
}

// -------------------------------------------------------------- prolongation
// u += P e, bilinear, e = 0 outside the coarse core; e[I][J] is coarse row I,
// column J, on fine row 2 I + 1, column 2 J + 1. One thread per fine cell
// (row y, column x), I = y >> 1, J = x >> 1:
//   odd row, odd column    p = e[I][J]
//   even row, odd column   p = 0.5 (e[I-1][J] + e[I][J])
//   odd row, even column   p = 0.5 (e[I][J-1] + e[I][J])
//   even row, even column  p = 0.25 ((e[I-1][J-1] + e[I][J-1]) + (e[I-1][J] + e[I][J]))
// Only core cells of e are read.
template <typename T>
__global__ __launch_bounds__(kMgBlock) void mg_prolong_add_kernel(const T* __restrict__ e, index_t cpitch,
                                                                  index_t ccore_off, index_t CW, index_t CH,
                                                                  T* __restrict__ u, index_t pitch, index_t core_off,
                                                                  index_t W, index_t H) {
  const index_t x = index_t(blockIdx.x) * 64 + (threadIdx.x & 63);
  const index_t y = index_t(blockIdx.y) * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const index_t I = y >> 1, J = x >> 1;
  auto at = [&](index_t i, index_t j) -> T {
    return (i >= 0 && i < CH && j >= 0 && j < CW) ? e[ccore_off + i * cpitch + j] : T(0);
  };
  T p;
  if (y & 1) {
    if (x & 1) p = at(I, J);
    else p = T(0.5) * (at(I, J - 1) + at(I, J));
  } else {
    if (x & 1) p = T(0.5) * (at(I - 1, J) + at(I, J));
    else p = T(0.25) * ((at(I - 1, J - 1) + at(I, J - 1)) + (at(I - 1, J) + at(I, J)));
  }
  T* q = u + core_off + y * pitch + x;
  *q = *q + p;
}

// -------------------------------------------------------------- coarse solve
// One workgroup: the whole W x H grid (both <= kMgCoarsestMax) plus a zero ring,
// double-buffered in LDS, with g beside it; `repeats` x tab.n sweeps from e = 0,
// one barrier per sweep; writes the core of e. Dynamic LDS:
// (2 (W + 2) (H + 2) + W H) elements.
template <typename T>
__global__ __launch_bounds__(kMgBlock) void mg_coarse_solve_kernel(const T* __restrict__ gsrc, T* __restrict__ e,
                                                                   index_t pitch, index_t core_off, int W, int H,
                                                                   int repeats, MgSweeps<T, kMaxLevels> tab, int levels) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mg_smem[];
  const int P = W + 2, FULL = P * (H + 2), N = W * H;
  T* a = reinterpret_cast<T*>(mg_smem);
  T* b = a + FULL;
  T* g = b + FULL;
  const int tid = threadIdx.x;
  for (int i = tid; i < 2 * FULL; i += kMgBlock) a[i] = T(0);
  for (int i = tid; i < N; i += kMgBlock) {
    const int r = i / W, c = i - r * W;
    g[i] = gsrc[core_off + index_t(r) * pitch + c];
  }
  __syncthreads();
  T* cur = a;
  T* nxt = b;
  for (int rep = 0; rep < repeats; ++rep) {
    for (int l = 0; l < levels; ++l) {
      const T ce = tab.center[l], nb = tab.neighbor[l], wt = tab.weight[l];
      for (int i = tid; i < N; i += kMgBlock) {
        const int r = i / W, c = i - r * W;
        const int q = (r + 1) * P + c + 1;
        nxt[q] = mg_sweep<T>(cur[q], cur[q - P], cur[q + P], cur[q - 1], cur[q + 1], g[i], ce, nb, wt);
      }
      __syncthreads();
      T* t = cur;
      cur = nxt;
      nxt = t;
    }
  }
  for (int i = tid; i < N; i += kMgBlock) {
    const int r = i / W, c = i - r * W;
    e[core_off + index_t(r) * pitch + c] = cur[(r + 1) * P + c + 1];
  }
}

}  // namespace detail
}  // namespace kernels
}  // namespace mxs
