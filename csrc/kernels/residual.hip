// Residual norms of the 5-point Jacobi update (kernels.hpp: stencil5_residual).
//
// For u' = A u the residual r = A u - u is the change the next single step
// would make: one streaming read of the tile, no write. Per core cell
//   r = fma(c_neighbor, (n + s) + (w + e), c_center * v) - v
// in the element type (the stencil kernels' expression, then one subtraction),
// reduced to max |r| and sum r^2 (accumulated in double).
//
// Shape (the RegisterRoll body of stencil_sweep.hpp with the store replaced
// by the two accumulations):
//   * a wave owns a strip of 64 16-byte lane vectors (256 fp32 / 128 fp64
//     columns), four waves side by side per workgroup, and walks a contiguous
//     band of rows with a rolling three-row register window in chunks of kCh
//     rows: the next chunk's loads are issued before the current chunk's
//     arithmetic, so each wave keeps kCh KiB in flight while it computes;
//   * x-neighbours come from the adjacent lane by DPP wave shifts; the one
//     column outside the strip on either side is one value per wave and row,
//     loaded through a wave-uniform address;
//   * the wave that holds the ragged last vector of a row (width % vector != 0)
//     and tiles that are not 16-byte aligned load element by element under
//     guards, never past column `width`;
//   * only the core and the ring cells beside it are read: row -1 and row
//     `height` over core columns only, column -1 and column `width` over core
//     rows only. Deeper ring layers, the corners and the alignment padding are
//     never loaded;
//   * plain global loads with 64-bit offsets: no buffer descriptor, so any tile
//     size works;
//   * rows are dealt to workgroups in contiguous bands (a multiple of kCh
//     rows): the only re-read is one row above and below each band.
// With a source tile g (u' = A u + g) the residual is r = (A u + g) - u: the
// stencil expression, then + g, then - v, each one rounded operation; g is read
// on core cells only.
// Deterministic: per-workgroup partials and a last-block finish in a fixed
// order (the dot_single_pass recipe of dot.hip: agent-scope release before the
// ticket, acquire after); no floating-point atomics. The grid depends only on
// the geometry and the CU count.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "mxs/core/error.hpp"
#include "mxs/kernels/kernels.hpp"
#include "mxs/runtime/hip_utils.hpp"

namespace mxs {
namespace kernels {
namespace {

constexpr int kResWaves = 4;                       // side by side along x
constexpr int kResBlock = kResWaves * kWaveSize;
constexpr int kCh = 4;                             // rows per chunk: row loads in flight per wave
constexpr int kResWgsPerCu = 4;                    // workgroups aimed at per CU (16 waves, all resident)

template <typename T>
struct ResVec {
  static constexpr int N = 16 / int(sizeof(T));
  using type = T __attribute__((ext_vector_type(N)));
};

// |x| as an unsigned bit pattern (absmax.hip): integer order is value order
// for non-negative IEEE values, and any NaN sorts above +inf.
__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
__device__ __forceinline__ unsigned long long abs_bits(double v) {
  return static_cast<unsigned long long>(__double_as_longlong(v)) & 0x7fffffffffffffffull;
}
__device__ __forceinline__ double from_bits(unsigned b) { return double(__uint_as_float(b)); }
__device__ __forceinline__ double from_bits(unsigned long long b) {
  return __longlong_as_double(static_cast<long long>(b));
}

template <typename T>
__device__ __forceinline__ T fma_t(T a, T b, T c) {
  if constexpr (sizeof(T) == 8) return __builtin_fma(a, b, c);
  else return __builtin_fmaf(a, b, c);
}

// Whole-wavefront DPP shifts (stencil_bodies.hpp): lane i reads lane i - 1
// (wave_shr) or lane i + 1 (wave_shl); the shifted-in lane gets 0.
constexpr int kDppWaveShl1 = 0x130;
constexpr int kDppWaveShr1 = 0x138;
template <int CTRL>
__device__ __forceinline__ float lane_shift(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ double lane_shift(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_mov_dpp(int(b & 0xffffffff), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_mov_dpp(int(b >> 32), CTRL, 0xf, 0xf, true);
  return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}

template <typename U>
__device__ __forceinline__ U umax(U a, U b) {
  return a > b ? a : b;
}

struct Pair {
  double sumsq;
  unsigned long long linf;  // bit pattern of a non-negative double (or a NaN)
};

// Workgroup reduction in a fixed order; valid in thread 0. lds: 2 * kResWaves slots.
__device__ __forceinline__ Pair block_reduce(Pair v, unsigned long long* lds) {
#pragma unroll
  for (int off = kWaveSize / 2; off > 0; off >>= 1) {
    v.sumsq += __shfl_xor(v.sumsq, off);
    v.linf = umax(v.linf, static_cast<unsigned long long>(__shfl_xor(static_cast<long long>(v.linf), off)));
  }
  const int lane = threadIdx.x & (kWaveSize - 1), wave = threadIdx.x / kWaveSize;
  if (lane == 0) {
    lds[2 * wave] = static_cast<unsigned long long>(__double_as_longlong(v.sumsq));
    lds[2 * wave + 1] = v.linf;
  }
  __syncthreads();
  Pair r{0.0, 0ull};
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kResWaves; ++w) {
      r.sumsq += __longlong_as_double(static_cast<long long>(lds[2 * w]));
      r.linf = umax(r.linf, lds[2 * w + 1]);
    }
  }
  return r;
}

// Grid: gx column groups (kResWaves strips each) x bands of band_rows rows,
// workgroup b = band * gx + group. partials: 2 doubles per workgroup.
// SRC: r = (A u + g) - u with g the core of the tile `gsrc` (same geometry),
// loaded beside each centre row at the centre row's own offsets and only where
// the centre vector holds core cells.
template <typename T, bool SRC>
__global__ __launch_bounds__(kResBlock) void stencil5_residual_kernel(const T* __restrict__ u, index_t pitch,
                                                                      index_t core_off, index_t W, index_t H,
                                                                      unsigned gx, index_t band_rows, T c0, T c1,
                                                                      int vec_ok, ResidualNorms* out,
                                                                      double* partials, unsigned* counter,
                                                                      const T* __restrict__ gsrc) {
  constexpr int N = ResVec<T>::N;
  constexpr index_t SEG = index_t(kWaveSize) * N;
  using V = typename ResVec<T>::type;
  using U = decltype(abs_bits(T(0)));

  const int lane = threadIdx.x & (kWaveSize - 1);
  const int wave = threadIdx.x / kWaveSize;
  const unsigned group = blockIdx.x % gx, band = blockIdx.x / gx;
  const index_t x = (index_t(group) * kResWaves + wave) * SEG + index_t(lane) * N;
  const index_t left_w = W - x;  // core columns from x on
  const int nvalid = left_w >= N ? N : (left_w > 0 ? int(left_w) : 0);
  const bool full = nvalid == N;
  const bool ragged = nvalid > 0 && nvalid < N;
  // The column just outside the strip: lane 0's left, and the right of the
  // strip's last whole vector (the next strip's first column, or column W of
  // the ring). A ragged vector carries its own right neighbour.
  const bool left_load = lane == 0 && nvalid > 0;
  const bool right_load = full && (lane == kWaveSize - 1 || left_w == N);
  const index_t y0 = index_t(band) * band_rows;
  const index_t y1 = y0 + band_rows < H ? y0 + band_rows : H;
  const T* __restrict__ p = u + core_off + x;

  // A wave is `fast` when the tile is 16-byte aligned and none of its lanes
  // holds a ragged vector (wave-uniform): then every vector load is
  // unconditional (lanes past the width read the strip's first vector again, a
  // cache hit, selected away) and the strip's two outside columns, one value
  // per wave and row each, come through wave-uniform addresses. The row loop
  // has no branch, so the next chunk's loads stay in flight under the current
  // chunk's arithmetic. Other waves (the one with the ragged vector, unaligned
  // tiles) load element by element under guards.
  const bool fast = vec_ok && __ballot(ragged) == 0;
  const index_t xs = (index_t(group) * kResWaves + __builtin_amdgcn_readfirstlane(wave)) * SEG;  // the strip's first column
  const index_t span = W - xs < SEG ? W - xs : SEG;  // its core columns (<= 0: the wave has none)
  const T* __restrict__ pf = full ? p : u + core_off + xs;
  const T* __restrict__ sl = u + core_off + xs - 1;     // wave-uniform: the column left of the strip
  const T* __restrict__ sr = u + core_off + xs + span;  // and right of its last core column

  // Row y of the strip. Core rows (`edge`) of a ragged vector also take the
  // element right of the last core column; ring rows stop at the core's width.
  auto ldv = [&](auto fast_tag, index_t y, bool edge) -> V {
    if constexpr (decltype(fast_tag)::value) {
      return __builtin_nontemporal_load(reinterpret_cast<const V*>(pf + y * pitch));
    } else {
      V v = V(T(0));
      const T* __restrict__ q = p + y * pitch;
      if (full) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = q[i];
      } else if (ragged) {
        const int cnt = nvalid + (edge ? 1 : 0);
#pragma unroll
        for (int i = 0; i < N; ++i)
          if (i < cnt) v[i] = q[i];
      }
      return v;
    }
  };
  // Row y (a core row) of the source tile: whole vectors of core cells, or the
  // ragged vector's core cells one by one.
  auto ldg = [&](auto fast_tag, index_t y) -> V {
    V v = V(T(0));
    if constexpr (SRC) {
      if constexpr (decltype(fast_tag)::value) {
        v = __builtin_nontemporal_load(reinterpret_cast<const V*>(gsrc + (pf - u) + y * pitch));
      } else {
        const T* __restrict__ q = gsrc + core_off + x + y * pitch;
#pragma unroll
        for (int i = 0; i < N; ++i)
          if (i < nvalid) v[i] = q[i];
      }
    }
    return v;
  };
  struct Edge {
    T l, r;
  };
  auto lde = [&](auto fast_tag, index_t y) -> Edge {  // core rows only
    if constexpr (decltype(fast_tag)::value) {
      return Edge{sl[y * pitch], sr[y * pitch]};
    } else {
      Edge e{T(0), T(0)};
      const T* __restrict__ q = p + y * pitch;
      if (left_load) e.l = q[-1];
      if (right_load) e.r = q[N];
      return e;
    }
  };

  U m = 0;
  double acc = 0.0;
  auto emit = [&](const V& up, const V& mid, const V& dn, Edge e, const V& gv) {
    T left = lane_shift<kDppWaveShr1>(mid[N - 1]);  // lane i - 1's last element
    T right = lane_shift<kDppWaveShl1>(mid[0]);      // lane i + 1's first
    left = lane == 0 ? e.l : left;
    right = right_load ? e.r : right;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const T w = i == 0 ? left : mid[i > 0 ? i - 1 : 0];
      const T ea = i == N - 1 ? right : mid[i < N - 1 ? i + 1 : 0];
      T r = fma_t<T>(c1, (up[i] + dn[i]) + (w + ea), c0 * mid[i]);
      if constexpr (SRC) r = r + gv[i];
      r = r - mid[i];
      r = i < nvalid ? r : T(0);  // a select: whatever sits past the core never enters
      m = umax<U>(m, abs_bits(r));
      acc = __builtin_fma(double(r), double(r), acc);
    }
  };

  // Rows [y0, y1) of the band: chunk c holds rows y + 1 .. y + kCh (the `down`
  // rows of rows y .. y + kCh - 1) with the outside columns of those that
  // become a centre row. While two whole chunks are left the body is
  // unguarded; the band's last rows run under row guards.
  struct Chunk {
    V v[kCh];
    Edge e[kCh];
    V g[SRC ? kCh : 1];  // the source beside the rows that become a centre row
  };
  auto walk = [&](auto fast_tag) {
    auto load = [&](index_t y, bool guarded) -> Chunk {
      Chunk c;
#pragma unroll
      for (int k = 0; k < kCh; ++k) {
        const index_t yn = y + k + 1;  // <= y1 <= H: row H of the ring at most
        c.v[k] = V(T(0));
        c.e[k] = Edge{T(0), T(0)};
        if (!guarded || yn <= y1) c.v[k] = ldv(fast_tag, yn, yn < H);
        if (!guarded || yn < y1) c.e[k] = lde(fast_tag, yn);
        if constexpr (SRC) {
          c.g[k] = V(T(0));
          if (!guarded || yn < y1) c.g[k] = ldg(fast_tag, yn);
        }
      }
      return c;
    };
    V up = ldv(fast_tag, y0 - 1, y0 > 0);
    V mid = ldv(fast_tag, y0, true);
    Edge emid = lde(fast_tag, y0);
    V gmid = ldg(fast_tag, y0);
    index_t y = y0;
    Chunk cur = load(y, true);
#pragma unroll 1
    for (; y + 2 * kCh < y1; y += kCh) {  // steady state: the next chunk's loads first
      const Chunk nxt = load(y + kCh, false);
#pragma unroll
      for (int k = 0; k < kCh; ++k) {
        emit(up, mid, cur.v[k], emid, gmid);
        up = mid;
        mid = cur.v[k];
        emid = cur.e[k];
        if constexpr (SRC) gmid = cur.g[k];
      }
      cur = nxt;
    }
#pragma unroll 1
    for (; y < y1; y += kCh) {
      Chunk nxt = cur;
      if (y + kCh < y1) nxt = load(y + kCh, true);
#pragma unroll
      for (int k = 0; k < kCh; ++k) {
        if (y + k < y1) emit(up, mid, cur.v[k], emid, gmid);
        up = mid;
        mid = cur.v[k];
        emid = cur.e[k];
        if constexpr (SRC) gmid = cur.g[k];
      }
      cur = nxt;
    }
  };
  if (y0 < y1 && span > 0) {  // wave-uniform (a wave past the width only joins the reduction)
    if (fast) walk(std::true_type{});
    else walk(std::false_type{});
  }

  // ONE __shared__ object (the "is last" flag shares the array, as in dot.hip).
  __shared__ unsigned long long lds[4 * kResWaves + 1];
  Pair mine{acc, static_cast<unsigned long long>(__double_as_longlong(from_bits(m)))};
  const Pair r = block_reduce(mine, lds);
  volatile unsigned* flag = reinterpret_cast<volatile unsigned*>(lds + 4 * kResWaves);
  if (threadIdx.x == 0) {
    partials[2 * index_t(blockIdx.x)] = r.sumsq;
    partials[2 * index_t(blockIdx.x) + 1] = __longlong_as_double(static_cast<long long>(r.linf));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the stores have left the wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // write back this XCD's L2 dirty lines
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag = (ticket == gridDim.x - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (*flag == 0u) return;  // workgroup-uniform
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // drop this CU's (possibly stale) L1 lines
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  Pair t{0.0, 0ull};
  for (unsigned i = threadIdx.x; i < gridDim.x; i += kResBlock) {  // fixed order per thread
    t.sumsq += partials[2 * index_t(i)];
    t.linf = umax(t.linf, static_cast<unsigned long long>(__double_as_longlong(partials[2 * index_t(i) + 1])));
  }
  const Pair total = block_reduce(t, lds + 2 * kResWaves);
  if (threadIdx.x == 0) {
    out->linf = __longlong_as_double(static_cast<long long>(total.linf));
    out->sumsq = total.sumsq;
  }
}

struct ResGrid {
  unsigned gx = 1;
  index_t bands = 1, band_rows = kCh;
};

// Column groups over the width, then enough row bands for ~kResWgsPerCu
// workgroups per CU; a band is a whole number of kCh-row chunks.
ResGrid residual_grid(const TileGeom& g, int elem_bytes) {
  ResGrid r;
  const index_t group_cols = index_t(kResWaves) * kWaveSize * (16 / elem_bytes);
  r.gx = unsigned(std::max<index_t>(1, (g.width + group_cols - 1) / group_cols));
  const index_t target = index_t(kResWgsPerCu) * std::max(1, device_cu_count());
  const index_t chunks = std::max<index_t>(1, (g.height + kCh - 1) / kCh);
  const index_t want = std::max<index_t>(1, std::min<index_t>(chunks, target / r.gx));
  r.band_rows = (chunks + want - 1) / want * kCh;
  r.bands = std::max<index_t>(1, (g.height + r.band_rows - 1) / r.band_rows);
  return r;
}

}  // namespace

int residual_grid_size(const TileGeom& g) {
  const ResGrid a = residual_grid(g, 4), b = residual_grid(g, 8);
  return int(std::max<index_t>(a.gx * a.bands, b.gx * b.bands));
}

template <typename T>
void stencil5_residual(const T* u, const TileGeom& g, Stencil5Coeffs c, ResidualNorms* out, double* partials,
                       unsigned* counter, hipStream_t s, const T* src) {
  MXS_CHECK(g.halo_x >= 1 && g.halo_y >= 1,
            "stencil5_residual: the tile has no ghost ring (it needs one at least 1 deep)");
  MXS_CHECK(g.width >= 0 && g.height >= 0 && g.pitch >= g.x_origin + g.total_width(),
            "stencil5_residual: bad tile geometry");
  MXS_CHECK(reinterpret_cast<std::uintptr_t>(u) % sizeof(T) == 0 &&
                reinterpret_cast<std::uintptr_t>(partials) % sizeof(double) == 0 &&
                reinterpret_cast<std::uintptr_t>(out) % sizeof(double) == 0 &&
                reinterpret_cast<std::uintptr_t>(counter) % sizeof(unsigned) == 0,
            "stencil5_residual: pointers must be element-aligned");
  if (g.width == 0 || g.height == 0) {  // no cells: both norms 0
    MXS_HIP_CHECK(hipMemsetAsync(out, 0, sizeof(ResidualNorms), s));
    return;
  }
  constexpr int N = ResVec<T>::N;
  const ResGrid rg = residual_grid(g, int(sizeof(T)));
  const index_t grid = index_t(rg.gx) * rg.bands;
  MXS_CHECK(grid <= index_t(residual_grid_size(g)) && grid < (index_t(1) << 31), "stencil5_residual: grid size");
  const int vec_ok = reinterpret_cast<std::uintptr_t>(u + g.core_offset()) % 16 == 0 && g.pitch % N == 0 &&
                     (src == nullptr || reinterpret_cast<std::uintptr_t>(src + g.core_offset()) % 16 == 0);
  MXS_CHECK(reinterpret_cast<std::uintptr_t>(src) % sizeof(T) == 0, "stencil5_residual: pointers must be element-aligned");
  // Re-initialise the ticket every call (a memset node under graph capture).
  MXS_HIP_CHECK(hipMemsetAsync(counter, 0, sizeof(unsigned), s));
  if (src)
    stencil5_residual_kernel<T, true><<<unsigned(grid), kResBlock, 0, s>>>(
        u, g.pitch, g.core_offset(), g.width, g.height, rg.gx, rg.band_rows, T(c.center), T(c.neighbor), vec_ok, out,
        partials, counter, src);
  else
    stencil5_residual_kernel<T, false><<<unsigned(grid), kResBlock, 0, s>>>(
        u, g.pitch, g.core_offset(), g.width, g.height, rg.gx, rg.band_rows, T(c.center), T(c.neighbor), vec_ok, out,
        partials, counter, nullptr);
  MXS_HIP_CHECK_LAUNCH();
}

template void stencil5_residual<float>(const float*, const TileGeom&, Stencil5Coeffs, ResidualNorms*, double*,
                                       unsigned*, hipStream_t, const float*);
template void stencil5_residual<double>(const double*, const TileGeom&, Stencil5Coeffs, ResidualNorms*, double*,
                                        unsigned*, hipStream_t, const double*);

}  // namespace kernels
}  // namespace mxs
