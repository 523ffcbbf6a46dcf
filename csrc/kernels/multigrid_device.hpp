// Device code of the multigrid kernels (kernels.hpp / multigrid.hip): the fused
// source-aware smoother, residual + full weighting, bilinear prolongation and
// the one-workgroup coarse solve. Plain launches: no cross-workgroup waits, no
// spin loops, no inline assembly.
//
// One kernel per step, two instantiations each. The multigrid solver's (mg_*)
// has a Dirichlet ring on every side; the V-cycle preconditioner's (mgp_*)
// carries a ghost code per side (pcg.hpp) and, in the smoother and the coarse
// solve, an optional start from zero and an optional dot epilogue. Which one a
// kernel is follows from the type of its table or sides argument: the plain
// types answer every side with a compile-time 0 and every epilogue pointer with
// a null, so the ghost code below folds away and the mg_* kernels are the code
// they were without it.
//
// Every expression below is a rounding contract with ops/multigrid.py and
// ops/pcg.py:
//   sweep        x' = fma(nb, (n + s) + (w + e), ce * c); x' = x' + T(w) * g
//                (the product rounded, then the sum);
//   residual     r = (fma(c1, (n + s) + (w + e), c0 * v) + g) - v;
//   restriction  g_c = (r_c + 0.5 ((rn + rs) + (rw + re))) + 0.25 ((rnw + rne) + (rsw + rse));
//   prolongation see mg_prolong_add_kernel;
//   ghost        beside an edge cell c of a reflecting side -c, an exact
//                negation, of a mirror side c itself, in the sweep and in the
//                residual;
//   dot          acc = fma(double(g), double(x'), acc) per thread in a fixed
//                order, then cg_reduce.hpp's grid reduction.
// The pragma keeps the compiler from contracting a product and a sum into an
// fma anywhere in this file; the fmas that are meant are written as builtins.
#pragma once

#include <hip/hip_runtime.h>

#include "cg_reduce.hpp"
#include "mxs/kernels/kernels.hpp"

#pragma clang fp contract(off)

namespace mxs {
namespace kernels {
namespace detail {

constexpr int kMgTw = 64, kMgTh = 32, kMgBlock = 256;
static_assert(kMgBlock == cgdev::kCgBlock, "the dot epilogue reduces over workgroups of kCgBlock threads");

template <typename T>
__device__ __forceinline__ T mg_fma(T a, T b, T c) {
  if constexpr (sizeof(T) == 8) return __builtin_fma(a, b, c);
  else return __builtin_fmaf(a, b, c);
}

template <typename T>
__device__ __forceinline__ T mg_sweep(T c, T n, T s, T w, T e, T g, T ce, T nb, T wt) {
  const T x = mg_fma<T>(nb, (n + s) + (w + e), ce * c);
  const T p = wt * g;
  return x + p;
}

// A level's four ghost codes (cg.hpp's GhostSides) as a kernel argument: 0 the
// ring, -1 reflect (minus the edge cell), +1 mirror (plus the edge cell).
struct MgpSides {
  int top, bottom, left, right;
  // The code that governs ghost row gy (column gx); 0 for every other row (column).
  __device__ __forceinline__ int row_code(index_t gy, index_t H) const { return gy == -1 ? top : (gy == H ? bottom : 0); }
  __device__ __forceinline__ int col_code(index_t gx, index_t W) const { return gx == -1 ? left : (gx == W ? right : 0); }
};
// The ring on every side, known to the compiler.
struct MgNoSides {
  static constexpr int top = 0, bottom = 0, left = 0, right = 0;
  __device__ __forceinline__ static constexpr int row_code(index_t, index_t) { return 0; }
  __device__ __forceinline__ static constexpr int col_code(index_t, index_t) { return 0; }
};

// The sides of a transfer kernel, whose argument list ends in (or holds) an
// MgpSides or nothing at all: the plain kernel keeps its argument list.
__device__ __forceinline__ MgNoSides mg_sides() { return {}; }
__device__ __forceinline__ MgpSides mg_sides(MgpSides sd) { return sd; }

// The ghost beside edge value v under a non-zero code: an exact negation or v itself.
template <typename T>
__device__ __forceinline__ T ghost_of(int code, T v) {
  return code < 0 ? -v : v;
}

// What the preconditioner's smoother and coarse solve get beside their sweeps:
// the sides and the dot epilogue's scalar block, partials and ticket.
struct MgpExtras {
  MgpSides sides;
  PcgScalars* sc;
  double* partials;
  unsigned* counter;
};
struct MgNoExtras {
  MgNoSides sides;
  static constexpr PcgScalars* sc = nullptr;
  static constexpr double* partials = nullptr;
  static constexpr unsigned* counter = nullptr;
};

// The sweep table of one launch, in the kernel arguments (a captured launch
// replays the same table): rounded to T once on the host. A kernel reads
// `tab.extras` of either table: the plain table's is a constant of the type and
// takes no room in the arguments (and no address of the argument: handing the
// table to a function instead moves the 1-sweep smoother's scalar loads), the
// preconditioner's is a member that hides it.
template <typename T, int N>
struct MgSweeps {
  T center[N];
  T neighbor[N];
  T weight[N];
  static constexpr MgNoExtras extras{};
};
template <typename T, int N>
struct MgpSweeps : MgSweeps<T, N> {
  MgpExtras extras;
};

// The dot epilogue's finish, in thread 0 of the workgroup that holds the total.
__device__ __forceinline__ void mg_store_rz(PcgScalars* sc, double sum) {
  if (sc->status != kCgRunning) return;  // the end of a solve: z is nobody's, nothing is stored
  const double rz_old = sc->rz;
  sc->beta = sc->iteration == 0 ? 0.0 : sum / rz_old;
  sc->rz = sum;
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
//
// A side with a ghost code stages its ghost row (column) from the core row
// (column) it reflects or mirrors, never from the tile's ring there. After
// sweep s the thread that advanced an edge cell also writes its ghost into the
// cell beside it: a ghost cell is advanced exactly when the cell it follows is,
// so it is valid to the same depth of the shrinking window. (The ghost cell of
// an advanced cell is always staged: r < LH - 1 - s gives r + 1 <= LH - 1.)
// Ghost corners and the ghost cells beside ring columns are never read by a
// core cell. DOT: the launch also sums g * x' of the last sweep over its output
// tile's core cells, both values in registers. ZERO: the iterate starts at 0
// and `in` is not read at all: every staged cell is the +0 (a reflecting ghost
// the -0) it would have read from a zeroed tile, so the bits are those of the
// plain launch on zeros (the first sweep gives 0 + T(w) g).
template <typename T, int NU, bool DOT, bool ZERO, typename Tab>
__global__ __launch_bounds__(kMgBlock) void mg_smooth_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                             const T* __restrict__ gsrc, index_t pitch,
                                                             index_t core_off, index_t W, index_t H, Tab tab) {
  constexpr int LW = kMgTw + 2 * NU, LH = kMgTh + 2 * NU;
  constexpr int LP = LW + 1;  // odd row pitch: column walks spread over the banks
  constexpr int IW = LW - 2, IH = LH - 2;  // cells that can advance (all but the staged edge)
  constexpr int CELLS = IW * IH;
  constexpr int PER = (CELLS + kMgBlock - 1) / kMgBlock;
  __shared__ T buf[LH * LP];

  const auto sd = tab.extras.sides;
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
    const cgdev::Total t = cgdev::grid_reduce_at(acc, 0ull, tab.extras.partials, tab.extras.counter, blockIdx.y * gridDim.x + blockIdx.x,
                                                 gridDim.x * gridDim.y);
    if (t.last && threadIdx.x == 0) mg_store_rz(tab.extras.sc, t.sum);
  }
}

// ------------------------------------------------- residual + full weighting
// A workgroup owns kMgCw x kMgCh coarse cells: it stages the fine u window
// (2 kMgCw + 3) x (2 kMgCh + 3) they reach, forms the fine residual of the
// (2 kMgCw + 1) x (2 kMgCh + 1) core cells in LDS (g read once per cell) and
// writes the weighted sums. No fine residual array leaves the workgroup.
// Any fine (W, H), coarse (CW, CH) with 2 CW + 1 <= W + 1: the fine residual
// of a cell outside the core is 0. With (W, H) odd and the coarse level
// ((W - 1) / 2, (H - 1) / 2) all nine fine cells of a coarse cell are core
// cells; with W even and CW = W / 2 the far neighbours of the last coarse cell
// (fine column W) are not, and likewise for rows. The ghost of a fine side with
// a code is staged from its edge row / column.
constexpr int kMgCw = 32, kMgCh = 16;

template <typename T, typename... Sides>
__global__ __launch_bounds__(kMgBlock) void mg_residual_restrict_kernel(const T* __restrict__ u,
                                                                        const T* __restrict__ gsrc, index_t pitch,
                                                                        index_t core_off, index_t W, index_t H,
                                                                        Sides... sides, T* __restrict__ gc, index_t cpitch,
                                                                        index_t ccore_off, index_t CW, index_t CH, T c0,
                                                                        T c1) {
  constexpr int RW = 2 * kMgCw + 1, RH = 2 * kMgCh + 1;  // fine residual cells
  constexpr int UW = RW + 2, UH = RH + 2;                // fine u cells staged
  constexpr int UP = UW, RP = RW;                        // both odd
  __shared__ T ub[UH * UP];
  __shared__ T rb[RH * RP];

  const auto sd = mg_sides(sides...);
  const index_t cx0 = index_t(blockIdx.x) * kMgCw, cy0 = index_t(blockIdx.y) * kMgCh;
  const index_t fx0 = 2 * cx0, fy0 = 2 * cy0;  // first fine residual cell
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
// u += P e, bilinear, e = 0 outside the coarse core; e[I][J] is coarse row I,
// column J, on fine row 2 I + 1, column 2 J + 1. One thread per fine cell
// (row y, column x), I = y >> 1, J = x >> 1:
//   odd row, odd column    p = e[I][J]
//   even row, odd column   p = 0.5 (e[I-1][J] + e[I][J])
//   odd row, even column   p = 0.5 (e[I][J-1] + e[I][J])
//   even row, even column  p = 0.25 ((e[I-1][J-1] + e[I][J-1]) + (e[I-1][J] + e[I][J]))
// Only core cells of e are read. A coarse ghost on a mirror side equals the
// mirrored coarse cell: at(i, j) clamps i = -1 -> 0 on a mirror top and i = CH ->
// CH - 1 on a mirror bottom, and the same for columns; on ring / reflect sides
// it stays 0.
template <typename T, typename... Sides>
__global__ __launch_bounds__(kMgBlock) void mg_prolong_add_kernel(const T* __restrict__ e, index_t cpitch,
                                                                  index_t ccore_off, index_t CW, index_t CH,
                                                                  T* __restrict__ u, index_t pitch, index_t core_off,
                                                                  index_t W, index_t H, Sides... sides) {
  const auto sd = mg_sides(sides...);
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
// One workgroup: the whole W x H grid (both <= kMgCoarsestMax) plus a zero ring,
// double-buffered in LDS, with g beside it; `repeats` x tab.n sweeps from e = 0,
// one barrier per sweep; writes the core of e. Dynamic LDS:
// (2 (W + 2) (H + 2) + W H) elements. On a side with a ghost code both buffers
// keep the ghost row (column) as the ghost of its edge row (column): -0 beside a
// reflecting side and +0 beside a mirror side at the start, then written by the
// thread that advances the edge cell. With a scalar block (a single-level
// preconditioner is this solve alone) it also sums src * e over the core and
// finishes like the smoother's dot: one workgroup, its own sum is the total.
template <typename T, typename Tab>
__global__ __launch_bounds__(kMgBlock) void mg_coarse_solve_kernel(const T* __restrict__ gsrc, T* __restrict__ e,
                                                                   index_t pitch, index_t core_off, int W, int H,
                                                                   int repeats, Tab tab, int levels) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mg_smem[];
  const int P = W + 2, FULL = P * (H + 2), N = W * H;
  T* a = reinterpret_cast<T*>(mg_smem);
  T* b = a + FULL;
  T* g = b + FULL;
  const auto sd = tab.extras.sides;
  const int tid = threadIdx.x;
  for (int i = tid; i < 2 * FULL; i += kMgBlock) {
    const int j = i < FULL ? i : i - FULL;
    const int r = j / P, c = j - r * P;  // ring included: core is 1..H, 1..W
    const bool in_cols = c >= 1 && c <= W, in_rows = r >= 1 && r <= H;
    const bool minus = (sd.bottom < 0 && r == H + 1 && in_cols) || (sd.right < 0 && c == W + 1 && in_rows);
    a[i] = minus ? -T(0) : T(0);
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
  if (tab.extras.sc == nullptr) return;  // grid-uniform
  __shared__ unsigned long long red[2 * cgdev::kCgWaves];
  const cgdev::Pair t = cgdev::block_reduce(cgdev::Pair{acc, 0ull}, red);
  if (tid == 0) mg_store_rz(tab.extras.sc, t.sum);
}

}  // namespace detail
}  // namespace kernels
}  // namespace mxs
