// Device code of the V-cycle preconditioner's kernels (kernels.hpp /
// pcg_precond.hip): the multigrid kernels of multigrid_device.hpp for any grid
// size, with the reflecting ghost of pcg.hpp. Plain launches: no cross-workgroup
// waits, no spin loops.
//
// Every expression is a rounding contract with ops/pcg.py, and is the one of
// multigrid_device.hpp:
//   sweep        x' = fma(nb, (n + s) + (w + e), ce * c); x' = x' + T(w) * g
//   residual     r = (fma(c1, (n + s) + (w + e), c0 * v) + g) - v
//   restriction  g_c = (r_c + 0.5 ((rn + rs) + (rw + re))) + 0.25 ((rnw + rne) + (rsw + rse))
//   ghost        on a reflecting side s (resp. e) of the last core row (column) is
//                -c, an exact negation, in the sweep and in the residual
//   dot          acc = fma(double(g), double(x'), acc) per thread in a fixed
//                order, then cg_reduce.hpp's grid reduction
// The pragma (set by multigrid_device.hpp for the rest of the translation unit)
// keeps the compiler from contracting a product and a sum anywhere here.
#pragma once

#include <hip/hip_runtime.h>

#include "cg_reduce.hpp"
#include "multigrid_device.hpp"

#pragma clang fp contract(off)

namespace mxs {
namespace kernels {
namespace detail {

static_assert(kMgBlock == cgdev::kCgBlock, "the dot epilogue reduces over workgroups of kCgBlock threads");

// A level's four ghost codes (cg.hpp's GhostSides) as a kernel argument: 0 the
// ring, -1 reflect (minus the edge cell), +1 mirror (plus the edge cell).
struct MgpSides {
  int top, bottom, left, right;
  // The code that governs ghost row gy (column gx); 0 for every other row (column).
  __device__ __forceinline__ int row_code(index_t gy, index_t H) const { return gy == -1 ? top : (gy == H ? bottom : 0); }
  __device__ __forceinline__ int col_code(index_t gx, index_t W) const { return gx == -1 ? left : (gx == W ? right : 0); }
};

// The ghost beside edge value v under a non-zero code: an exact negation or v itself.
template <typename T>
__device__ __forceinline__ T ghost_of(int code, T v) {
  return code < 0 ? -v : v;
}

// ------------------------------------------------------------------ smoother
// mg_smooth_kernel with ghost codes (reflect described here; a mirror side, near
// or far, is the same with the other sign: the ghost row -1 / column -1 mirrors
// core row 0 / column 0 and the ZERO start stages +0 there).
// The staged window holds the ghost row H
// (column W) of a reflecting side as minus the staged core row H - 1 (column
// W - 1), never the tile's ring there. After sweep s the thread that advanced
// a cell of the last core row (column) also writes its negation into the ghost
// cell beside it: a ghost cell is advanced exactly when the cell it mirrors is,
// so it is valid to the same depth of the shrinking window. (The ghost cell of
// an advanced cell is always staged: r < LH - 1 - s gives r + 1 <= LH - 1.)
// Ghost corners and the ghost cells beside ring columns are never read by a
// core cell. DOT: the launch also sums g * x' of the last sweep over its output
// tile's core cells, both values in registers. ZERO: the iterate starts at 0
// and `in` is not read at all: every staged cell is the +0 (a reflecting ghost
// the -0) it would have read from a zeroed tile, so the bits are those of the
// plain launch on zeros (the first sweep gives 0 + T(w) g).
template <typename T, int NU, bool DOT, bool ZERO>
__global__ __launch_bounds__(kMgBlock) void mgp_smooth_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                              const T* __restrict__ gsrc, index_t pitch,
                                                              index_t core_off, index_t W, index_t H,
                                                              MgSweeps<T, NU> tab, MgpSides sd, PcgScalars* sc,
                                                              double* partials, unsigned* counter) {
  constexpr int LW = kMgTw + 2 * NU, LH = kMgTh + 2 * NU;
  constexpr int LP = LW + 1;
  constexpr int IW = LW - 2, IH = LH - 2;
  constexpr int CELLS = IW * IH;
  constexpr int PER = (CELLS + kMgBlock - 1) / kMgBlock;
  __shared__ T buf[LH * LP];

  const index_t tx0 = index_t(blockIdx.x) * kMgTw, ty0 = index_t(blockIdx.y) * kMgTh;
  const int tid = threadIdx.x;

  for (int i = tid; i < LH * LW; i += kMgBlock) {
    const int r = i / LW, c = i - r * LW;
    const index_t gy = ty0 - NU + r, gx = tx0 - NU + c;
    T v = T(0);
    if (gy >= -1 && gy <= H && gx >= -1 && gx <= W) {
      const int cy = sd.row_code(gy, H), cx = sd.col_code(gx, W);
      if (cy == 0 && cx == 0) {
        if constexpr (!ZERO) v = in[core_off + gy * pitch + gx];
      } else if (cy != 0 && cx == 0) {
        if (gx >= 0 && gx < W) v = ghost_of<T>(cy, ZERO ? T(0) : in[core_off + (gy < 0 ? 0 : H - 1) * pitch + gx]);
      } else if (cx != 0 && cy == 0) {
        if (gy >= 0 && gy < H) v = ghost_of<T>(cx, ZERO ? T(0) : in[core_off + gy * pitch + (gx < 0 ? 0 : W - 1)]);
      }
    }
    buf[r * LP + c] = v;
  }

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

  double acc = 0.0;
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
        if (r > s && r < LH - 1 - s && c > s && c < LW - 1 - s) {
          buf[r * LP + c] = res[k];
          const index_t gy = ty0 - NU + r, gx = tx0 - NU + c;
          if (sd.bottom && gy == H - 1) buf[(r + 1) * LP + c] = ghost_of<T>(sd.bottom, res[k]);
          if (sd.right && gx == W - 1) buf[r * LP + c + 1] = ghost_of<T>(sd.right, res[k]);
          if (sd.top && gy == 0) buf[(r - 1) * LP + c] = ghost_of<T>(sd.top, res[k]);
          if (sd.left && gx == 0) buf[r * LP + c - 1] = ghost_of<T>(sd.left, res[k]);
          if constexpr (DOT) {
            // The output tile's cells (live: inside the core), at the last sweep.
            if (s == NU - 1 && r >= NU && r < NU + kMgTh && c >= NU && c < NU + kMgTw)
              acc = __builtin_fma(double(gv[k]), double(res[k]), acc);
          }
        }
      }
    }
    __syncthreads();
  }

  for (int i = tid; i < kMgTh * kMgTw; i += kMgBlock) {
    const int r = i / kMgTw, c = i - r * kMgTw;
    const index_t gy = ty0 + r, gx = tx0 + c;
    if (gy < H && gx < W) out[core_off + gy * pitch + gx] = buf[(r + NU) * LP + c + NU];
  }

  if constexpr (DOT) {
    const cgdev::Total t = cgdev::grid_reduce_at(acc, 0ull, partials, counter, blockIdx.y * gridDim.x + blockIdx.x,
                                                 gridDim.x * gridDim.y);
    if (!t.last || threadIdx.x != 0) return;
    if (sc->status != kCgRunning) return;  // the end of a solve: z is nobody's, nothing is stored
    const double rz_old = sc->rz;
    sc->beta = sc->iteration == 0 ? 0.0 : t.sum / rz_old;
    sc->rz = t.sum;
  }
}

// ------------------------------------------------- residual + full weighting
// mg_residual_restrict_kernel for any fine (W, H), coarse (W / 2, H / 2). The
// fine residual of a cell outside the core is 0: on an even side those are the
// far neighbours of the last coarse cell (fine column W, row H). The ghost of a
// reflecting fine level is staged as minus its last core row / column.
template <typename T>
__global__ __launch_bounds__(kMgBlock) void mgp_residual_restrict_kernel(const T* __restrict__ u,
                                                                         const T* __restrict__ gsrc, index_t pitch,
                                                                         index_t core_off, index_t W, index_t H,
                                                                         MgpSides sd, T* __restrict__ gc, index_t cpitch,
                                                                         index_t ccore_off, index_t CW, index_t CH,
                                                                         T c0, T c1) {
  constexpr int RW = 2 * kMgCw + 1, RH = 2 * kMgCh + 1;
  constexpr int UW = RW + 2, UH = RH + 2;
  constexpr int UP = UW, RP = RW;
  __shared__ T ub[UH * UP];
  __shared__ T rb[RH * RP];

  const index_t cx0 = index_t(blockIdx.x) * kMgCw, cy0 = index_t(blockIdx.y) * kMgCh;
  const index_t fx0 = 2 * cx0, fy0 = 2 * cy0;
  const int tid = threadIdx.x;

  for (int i = tid; i < UH * UW; i += kMgBlock) {
    const int r = i / UW, c = i - r * UW;
    const index_t gy = fy0 - 1 + r, gx = fx0 - 1 + c;  // >= -1 always
    T v = T(0);
    if (gy <= H && gx <= W) {
      const int cy = sd.row_code(gy, H), cx = sd.col_code(gx, W);
      if (cy == 0 && cx == 0) {
        v = u[core_off + gy * pitch + gx];
      } else if (cy != 0 && cx == 0) {
        if (gx >= 0 && gx < W) v = ghost_of<T>(cy, u[core_off + (gy < 0 ? 0 : H - 1) * pitch + gx]);
      } else if (cx != 0 && cy == 0) {
        if (gy >= 0 && gy < H) v = ghost_of<T>(cx, u[core_off + gy * pitch + (gx < 0 ? 0 : W - 1)]);
      }
    }
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
      // The transpose of the mirrored prolongation: a fine row / column whose outer
      // coarse neighbour is a mirror ghost counts twice (an exact doubling).
      if ((sd.top > 0 && gy == 0) || (sd.bottom > 0 && gy == H - 1 && (H & 1))) res = res + res;
      if ((sd.left > 0 && gx == 0) || (sd.right > 0 && gx == W - 1 && (W & 1))) res = res + res;
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
// mg_prolong_add_kernel where a coarse ghost on a mirror side equals the
// mirrored coarse cell: at(i, j) clamps i = -1 -> 0 on a mirror top and i = CH ->
// CH - 1 on a mirror bottom, and the same for columns; on ring / reflect sides
// it stays 0. The expressions are mg_prolong_add_kernel's.
template <typename T>
__global__ __launch_bounds__(kMgBlock) void mgp_prolong_add_kernel(const T* __restrict__ e, index_t cpitch,
                                                                   index_t ccore_off, index_t CW, index_t CH,
                                                                   T* __restrict__ u, index_t pitch, index_t core_off,
                                                                   index_t W, index_t H, MgpSides sd) {
  const index_t x = index_t(blockIdx.x) * 64 + (threadIdx.x & 63);
  const index_t y = index_t(blockIdx.y) * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const index_t I = y >> 1, J = x >> 1;
  auto at = [&](index_t i, index_t j) -> T {
    if (sd.top > 0 && i < 0) i = 0;
    if (sd.bottom > 0 && i >= CH) i = CH - 1;
    if (sd.left > 0 && j < 0) j = 0;
    if (sd.right > 0 && j >= CW) j = CW - 1;
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
// mg_coarse_solve_kernel with ghost codes (a mirror side like a reflecting one,
// with +0 at the start and the advanced edge cell itself afterwards): both LDS buffers keep the ghost row
// H (column W) of a reflecting side as minus the last core row (column): -0 at
// the start, then written by the thread that advances the mirrored cell. With
// `sc` it also sums src * e over the core and finishes like mgp_smooth's dot.
template <typename T>
__global__ __launch_bounds__(kMgBlock) void mgp_coarse_solve_kernel(const T* __restrict__ gsrc, T* __restrict__ e,
                                                                    index_t pitch, index_t core_off, int W, int H,
                                                                    int repeats, MgSweeps<T, kMaxLevels> tab, int levels,
                                                                    MgpSides sd, PcgScalars* sc) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mgp_smem[];
  const int P = W + 2, FULL = P * (H + 2), N = W * H;
  T* a = reinterpret_cast<T*>(mgp_smem);
  T* b = a + FULL;
  T* g = b + FULL;
  const int tid = threadIdx.x;
  for (int i = tid; i < 2 * FULL; i += kMgBlock) {
    const int j = i < FULL ? i : i - FULL;
    const int r = j / P, c = j - r * P;  // ring included: core is 1..H, 1..W
    const bool in_cols = c >= 1 && c <= W, in_rows = r >= 1 && r <= H;
    const bool minus = (sd.bottom < 0 && r == H + 1 && in_cols) || (sd.right < 0 && c == W + 1 && in_rows);
    a[i] = minus ? -T(0) : T(0);  // a mirror ghost starts at +0
  }
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
        const T v = mg_sweep<T>(cur[q], cur[q - P], cur[q + P], cur[q - 1], cur[q + 1], g[i], ce, nb, wt);
        nxt[q] = v;
        if (sd.bottom && r == H - 1) nxt[q + P] = ghost_of<T>(sd.bottom, v);
        if (sd.right && c == W - 1) nxt[q + 1] = ghost_of<T>(sd.right, v);
        if (sd.top && r == 0) nxt[q - P] = ghost_of<T>(sd.top, v);
        if (sd.left && c == 0) nxt[q - 1] = ghost_of<T>(sd.left, v);
      }
      __syncthreads();
      T* t = cur;
      cur = nxt;
      nxt = t;
    }
  }
  double acc = 0.0;
  for (int i = tid; i < N; i += kMgBlock) {
    const int r = i / W, c = i - r * W;
    const T v = cur[(r + 1) * P + c + 1];
    e[core_off + index_t(r) * pitch + c] = v;
    acc = __builtin_fma(double(g[i]), double(v), acc);
  }
  // A single-level preconditioner is this solve alone: it then carries the dot
  // epilogue of mgp_smooth (one workgroup: its own sum is the total).
  if (sc == nullptr) return;  // grid-uniform
  __shared__ unsigned long long red[2 * cgdev::kCgWaves];
  const cgdev::Pair t = cgdev::block_reduce(cgdev::Pair{acc, 0ull}, red);
  if (tid != 0 || sc->status != kCgRunning) return;
  const double rz_old = sc->rz;
  sc->beta = sc->iteration == 0 ? 0.0 : t.sum / rz_old;
  sc->rz = t.sum;
}

}  // namespace detail
}  // namespace kernels
}  // namespace mxs
