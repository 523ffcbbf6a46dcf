// The three kernels of conjugate gradients for L u = b (kernels.hpp: cg_start,
// cg_apply, cg_update; mxs/kernels/cg.hpp; docs/ARCHITECTURE.md "Conjugate
// gradients"). One CG iteration is cg_apply + cg_update: the direction update
// rides in the operator's pass and every dot product in the pass that makes
// its terms, so an iteration streams 10 element arrays (apply: r, p_old in,
// p_new, q out; update: u, r, p, q in, u, r out) and never a reduction pass.
// The same three bodies, instantiated on PcgScalars, are pcg_start, pcg_apply
// and pcg_update of multigrid-preconditioned CG (mxs/kernels/pcg.hpp): z = M r
// stands for r in apply, alpha = rz / pq, and beta comes from the
// preconditioner's dot epilogue (multigrid_device.hpp) instead of update.
// cg_heat_start / pcg_heat_start are the start kernel of an implicit heat step
// (mxs/kernels/heat.hpp): the step's right-hand side g is made and stored in
// the pass that takes the first residual, a kernel of its own so that
// cg_start_kernel's instantiations stay as they are.
//
// Shape (that of residual.hip):
//   * a lane owns one 16-byte vector (4 fp32 / 2 fp64 columns), a wave a strip
//     of 64 of them, four waves side by side per workgroup, which walks a
//     contiguous band of rows with a rolling three-row register window in
//     chunks of kCh rows whose loads are all issued before the arithmetic;
//   * x-neighbours come from the adjacent lane by DPP wave shifts; the one
//     column outside the strip on either side is one value per wave and row;
//   * whole vectors of an aligned tile move as 16-byte loads and stores, the
//     ragged last vector of a row (width % vector != 0) and unaligned tiles
//     element by element under guards, never past column `width`;
//   * plain global accesses with 64-bit offsets, so any tile size works;
//   * cg_apply never loads outside the core of r or p_old: p_new is 0 there.
//     cg_start reads the ring cells beside the core of u only (row -1 and row
//     `height` over core columns, column -1 and `width` over core rows).
// Deterministic: per-workgroup partials and a last-block finish in a fixed
// order (agent-scope release before the ticket, acquire after it, partials read
// on the vector path); no floating-point atomics; the grid depends only on the
// geometry and the CU count. The last workgroup alone writes the scalar block
// and puts the ticket back to 0; every workgroup reads status (and alpha or
// beta) once at entry, so no launch writes what the same launch reads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <type_traits>

#include "mxs/core/error.hpp"
#include "mxs/kernels/kernels.hpp"
#include "mxs/runtime/hip_utils.hpp"
#include "cg_reduce.hpp"

// Every expression below is a rounding contract with ops/cg.py: the fused
// multiply-adds that are meant are builtins, nothing else may be contracted.
#pragma clang fp contract(off)

namespace mxs {
namespace kernels {
namespace {

using namespace cgdev;

constexpr int kCh = 4;         // rows per chunk: row loads in flight per wave and array
// Workgroups aimed at per CU. Every workgroup ends in an agent-scope release (a
// write-back of its XCD's L2, which these kernels' own stores keep dirty), so
// the count of workgroups is a cost of its own: measured on an MI355X at 2048^2
// .. 8192^2, 1 per CU takes 0.50 .. 0.93 of the time of 4 per CU and more are
// slower still (docs/PERF.md "Conjugate gradients").
constexpr int kCgWgsPerCu = 1;
// The mirror (Neumann) sides of a launch as one kernel argument.
constexpr int kMirrorTop = 1, kMirrorBottom = 2, kMirrorLeft = 4, kMirrorRight = 8;

std::atomic<const char*> g_last_cg{""};

template <typename T>
struct CgVec {
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

// The chosen norm of (rr, linf) against tol.
__device__ __forceinline__ bool cg_within(int norm, double rr, double linf, double tol) {
  return norm == kCgNormLinf ? linf <= tol : __builtin_sqrt(rr) <= tol;
}

// A lane's place in the launch: workgroup b = band * gx + group; its vector
// starts at core column x and holds nvalid core columns (0: past the width).
template <typename T>
struct Strip {
  static constexpr int N = CgVec<T>::N;
  using V = typename CgVec<T>::type;
  int lane;
  index_t pitch, W, H, x, y0, y1;
  int nvalid;
  bool vec, full, left_load, right_load, any;

  __device__ __forceinline__ Strip(index_t pitch_, index_t W_, index_t H_, unsigned gx, index_t band_rows, int vec_ok)
      : pitch(pitch_), W(W_), H(H_) {
    lane = threadIdx.x & (kWaveSize - 1);
    const int wave = threadIdx.x / kWaveSize;
    const unsigned group = blockIdx.x % gx, band = blockIdx.x / gx;
    constexpr index_t SEG = index_t(kWaveSize) * N;
    x = (index_t(group) * kCgWaves + wave) * SEG + index_t(lane) * N;
    const index_t left_w = W - x;  // core columns from x on
    nvalid = left_w >= N ? N : (left_w > 0 ? int(left_w) : 0);
    full = nvalid == N;
    vec = vec_ok != 0;
    // The column just outside the strip: lane 0's left, and the right of the
    // strip's last whole vector. A ragged vector carries its own right neighbour.
    left_load = lane == 0 && nvalid > 0;
    right_load = full && (lane == kWaveSize - 1 || left_w == N);
    y0 = index_t(band) * band_rows;
    y1 = y0 + band_rows < H ? y0 + band_rows : H;
    const index_t xs = (index_t(group) * kCgWaves + __builtin_amdgcn_readfirstlane(wave)) * SEG;
    any = y0 < y1 && xs < W;  // wave-uniform: a wave past the width only joins the reduction
  }
  // Elements [x, x + cnt) of row y of the tile whose core starts at `c`, the rest 0.
  __device__ __forceinline__ V ld(const T* c, index_t y, int cnt) const {
    V v = V(T(0));
    const T* q = c + y * pitch + x;
    if (vec && cnt >= N) {
      v = *reinterpret_cast<const V*>(q);
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i)
        if (i < cnt) v[i] = q[i];
    }
    return v;
  }
  // The core elements of the vector to row y.
  __device__ __forceinline__ void st(T* c, index_t y, const V& v) const {
    T* q = c + y * pitch + x;
    if (vec && full) {
      *reinterpret_cast<V*>(q) = v;
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i)
        if (i < nvalid) q[i] = v[i];
    }
  }
};

template <typename T>
struct Edge {
  T l, r;
};

// ------------------------------------------------------------------ cg_start
// S: CgScalars (cg_*) or PcgScalars (pcg_*: no first direction is stored, rz = 0).
// NEU: some side is a mirror (`mirror`: kMirrorTop | ...); without it the code is the ring-only kernel's.
template <typename T, typename S, bool NEU>
__global__ __launch_bounds__(kCgBlock) void cg_start_kernel(const T* __restrict__ u, const T* __restrict__ g,
                                                            T* __restrict__ r, T* __restrict__ p, index_t pitch,
                                                            index_t core_off, index_t W, index_t H, unsigned gx,
                                                            index_t band_rows, T c0, T c1, int vec_ok, int mirror, S* sc,
                                                            double* partials, unsigned* counter) {
  constexpr bool kPcg = std::is_same<S, PcgScalars>::value;
  constexpr int N = CgVec<T>::N;
  using V = typename CgVec<T>::type;
  using U = decltype(abs_bits(T(0)));
  const Strip<T> L(pitch, W, H, gx, band_rows, vec_ok);
  const T* uc = u + core_off;
  const T* gc = g + core_off;
  T* rc = r + core_off;
  T* pc = p + core_off;
  const int nvalid = L.nvalid;

  // Row y of u: ring rows stop at the core's width, core rows of a ragged
  // vector also take the element right of the last core column.
  auto ldu = [&](index_t y) -> V {
    const bool core_row = y >= 0 && y < H;
    return L.ld(uc, y, nvalid == 0 ? 0 : (nvalid < N && core_row ? nvalid + 1 : nvalid));
  };
  auto lde = [&](index_t y) -> Edge<T> {  // core rows only
    Edge<T> e{T(0), T(0)};
    const T* q = uc + y * pitch + L.x;
    if (L.left_load) e.l = q[-1];
    if (L.right_load) e.r = q[N];
    return e;
  };

  U m = 0;
  double acc = 0.0;
  if (L.any) {
    V up = ldu(L.y0 - 1), mid = ldu(L.y0);
    Edge<T> emid = lde(L.y0);
    V gmid = L.ld(gc, L.y0, nvalid);
#pragma unroll 1
    for (index_t y = L.y0; y < L.y1; y += kCh) {
      V dn[kCh], gn[kCh];
      Edge<T> en[kCh];
#pragma unroll
      for (int k = 0; k < kCh; ++k) {  // rows y + 1 .. y + kCh: row y1 <= H at most
        const index_t yn = y + k + 1;
        dn[k] = V(T(0));
        gn[k] = V(T(0));
        en[k] = Edge<T>{T(0), T(0)};
        if (yn <= L.y1) dn[k] = ldu(yn);
        if (yn < L.y1) {
          en[k] = lde(yn);
          gn[k] = L.ld(gc, yn, nvalid);
        }
      }
#pragma unroll
      for (int k = 0; k < kCh; ++k) {
        if (y + k < L.y1) {
          T left = lane_shift<kDppWaveShr1>(mid[N - 1]);  // lane i - 1's last element
          T right = lane_shift<kDppWaveShl1>(mid[0]);      // lane i + 1's first
          left = L.lane == 0 ? emid.l : left;
          right = L.right_load ? emid.r : right;
          V out;
#pragma unroll
          for (int i = 0; i < N; ++i) {
            const T w = i == 0 ? left : mid[i > 0 ? i - 1 : 0];
            const T ea = i == N - 1 ? right : mid[i < N - 1 ? i + 1 : 0];
            T res;
            if constexpr (NEU) {  // a mirror ghost is edge + ring (the ring holds d), one addition
              const T c = mid[i];
              const T nn = (mirror & kMirrorTop) && y + k == 0 ? c + up[i] : up[i];
              const T ss = (mirror & kMirrorBottom) && y + k == H - 1 ? c + dn[k][i] : dn[k][i];
              const T ww = (mirror & kMirrorLeft) && L.x + i == 0 ? c + w : w;
              const T ee = (mirror & kMirrorRight) && L.x + i == W - 1 ? c + ea : ea;
              res = fma_t<T>(c1, (nn + ss) + (ww + ee), c0 * c);
            } else {
              res = fma_t<T>(c1, (up[i] + dn[k][i]) + (w + ea), c0 * mid[i]);
            }
            res = res + gmid[i];
            res = res - mid[i];
            res = i < nvalid ? res : T(0);  // a select: whatever sits past the core never enters
            out[i] = res;
            m = umax<U>(m, abs_bits(res));
            acc = __builtin_fma(double(res), double(res), acc);
          }
          L.st(rc, y + k, out);
          if constexpr (!kPcg) L.st(pc, y + k, out);
        }
        up = mid;
        mid = dn[k];
        emid = en[k];
        gmid = gn[k];
      }
    }
  }

  const Total t = grid_reduce(acc, static_cast<unsigned long long>(__double_as_longlong(from_bits(m))), partials, counter);
  if (!t.last || threadIdx.x != 0) return;
  const int max_iters = sc->max_iters;
  sc->rr = t.sum;
  sc->linf = t.linf;
  if constexpr (kPcg) sc->rz = 0.0;
  sc->pq = 0.0;
  sc->alpha = 0.0;
  sc->beta = 0.0;
  sc->iteration = 0;
  sc->status = cg_within(sc->norm, t.sum, t.linf, sc->tol) ? kCgConverged : (max_iters <= 0 ? kCgMaxIters : kCgRunning);
}

// ------------------------------------------------------------- cg_heat_start
// The start of an implicit heat step (mxs/kernels/heat.hpp): cg_start_kernel
// with the right-hand side made in the same pass. Per core cell, with S the
// neighbour sum as cg_start forms it (ghosts included),
//   g = fma(b, S, a c) (+ s q with SRC: the product rounded, then the sum)
//   r = (fma(c1, S, 0 c) + g) - c
// so r, rr and linf are those of cg_start_kernel on (u, the stored g) with
// c0 = 0: same grid, same partials, same finish. Writes the cores of g, r (and
// p); reads u as cg_start does and, with SRC, the core of q.
template <typename T, typename S, bool NEU, bool SRC>
__global__ __launch_bounds__(kCgBlock) void cg_heat_start_kernel(const T* __restrict__ u, const T* __restrict__ q,
                                                                 T* __restrict__ g, T* __restrict__ r,
                                                                 T* __restrict__ p, index_t pitch, index_t core_off,
                                                                 index_t W, index_t H, unsigned gx, index_t band_rows,
                                                                 T c1, T ha, T hb, T hs, int vec_ok, int mirror, S* sc,
                                                                 double* partials, unsigned* counter) {
  constexpr bool kPcg = std::is_same<S, PcgScalars>::value;
  constexpr int N = CgVec<T>::N;
  constexpr int kQ = SRC ? kCh : 1;  // no source: nothing of q is held or read
  using V = typename CgVec<T>::type;
  using U = decltype(abs_bits(T(0)));
  const Strip<T> L(pitch, W, H, gx, band_rows, vec_ok);
  const T* uc = u + core_off;
  const T* qc = q + core_off;
  T* gc = g + core_off;
  T* rc = r + core_off;
  T* pc = p + core_off;
  const int nvalid = L.nvalid;

  // Row y of u and its edge columns: cg_start_kernel's.
  auto ldu = [&](index_t y) -> V {
    const bool core_row = y >= 0 && y < H;
    return L.ld(uc, y, nvalid == 0 ? 0 : (nvalid < N && core_row ? nvalid + 1 : nvalid));
  };
  auto lde = [&](index_t y) -> Edge<T> {  // core rows only
    Edge<T> e{T(0), T(0)};
    const T* a = uc + y * pitch + L.x;
    if (L.left_load) e.l = a[-1];
    if (L.right_load) e.r = a[N];
    return e;
  };

  U m = 0;
  double acc = 0.0;
  if (L.any) {
    V up = ldu(L.y0 - 1), mid = ldu(L.y0);
    Edge<T> emid = lde(L.y0);
    V qmid = V(T(0));
    if constexpr (SRC) qmid = L.ld(qc, L.y0, nvalid);
#pragma unroll 1
    for (index_t y = L.y0; y < L.y1; y += kCh) {
      V dn[kCh], qn[kQ];
      Edge<T> en[kCh];
#pragma unroll
      for (int k = 0; k < kCh; ++k) {  // rows y + 1 .. y + kCh: row y1 <= H at most
        const index_t yn = y + k + 1;
        dn[k] = V(T(0));
        en[k] = Edge<T>{T(0), T(0)};
        if constexpr (SRC) qn[k] = V(T(0));
        if (yn <= L.y1) dn[k] = ldu(yn);
        if (yn < L.y1) {
          en[k] = lde(yn);
          if constexpr (SRC) qn[k] = L.ld(qc, yn, nvalid);
        }
      }
#pragma unroll
      for (int k = 0; k < kCh; ++k) {
        if (y + k < L.y1) {
          T left = lane_shift<kDppWaveShr1>(mid[N - 1]);  // lane i - 1's last element
          T right = lane_shift<kDppWaveShl1>(mid[0]);      // lane i + 1's first
          left = L.lane == 0 ? emid.l : left;
          right = L.right_load ? emid.r : right;
          V out, gout;
#pragma unroll
          for (int i = 0; i < N; ++i) {
            const T w = i == 0 ? left : mid[i > 0 ? i - 1 : 0];
            const T ea = i == N - 1 ? right : mid[i < N - 1 ? i + 1 : 0];
            const T c = mid[i];
            T sum;
            if constexpr (NEU) {  // a mirror ghost is edge + ring (the ring holds d), one addition
              const T nn = (mirror & kMirrorTop) && y + k == 0 ? c + up[i] : up[i];
              const T ss = (mirror & kMirrorBottom) && y + k == H - 1 ? c + dn[k][i] : dn[k][i];
              const T ww = (mirror & kMirrorLeft) && L.x + i == 0 ? c + w : w;
              const T ee = (mirror & kMirrorRight) && L.x + i == W - 1 ? c + ea : ea;
              sum = (nn + ss) + (ww + ee);
            } else {
              sum = (up[i] + dn[k][i]) + (w + ea);
            }
            T gv = fma_t<T>(hb, sum, ha * c);
            if constexpr (SRC) gv = gv + hs * qmid[i];
            T res = fma_t<T>(c1, sum, T(0) * c);
            res = res + gv;
            res = res - c;
            res = i < nvalid ? res : T(0);  // a select: whatever sits past the core never enters
            gout[i] = gv;
            out[i] = res;
            m = umax<U>(m, abs_bits(res));
            acc = __builtin_fma(double(res), double(res), acc);
          }
          L.st(gc, y + k, gout);
          L.st(rc, y + k, out);
          if constexpr (!kPcg) L.st(pc, y + k, out);
        }
        up = mid;
        mid = dn[k];
        emid = en[k];
        if constexpr (SRC) qmid = qn[k];
      }
    }
  }

  const Total t = grid_reduce(acc, static_cast<unsigned long long>(__double_as_longlong(from_bits(m))), partials, counter);
  if (!t.last || threadIdx.x != 0) return;
  const int max_iters = sc->max_iters;
  sc->rr = t.sum;
  sc->linf = t.linf;
  if constexpr (kPcg) sc->rz = 0.0;
  sc->pq = 0.0;
  sc->alpha = 0.0;
  sc->beta = 0.0;
  sc->iteration = 0;
  sc->status = cg_within(sc->norm, t.sum, t.linf, sc->tol) ? kCgConverged : (max_iters <= 0 ? kCgMaxIters : kCgRunning);
}

// ------------------------------------------------------------------ cg_apply
// S: CgScalars (alpha = rr / pq) or PcgScalars (r is z = M r, alpha = rz / pq).
// NEU: on a mirror side the ghost operand is the edge value of p_new itself (the ring is folded into b).
template <typename T, typename S, bool NEU>
__global__ __launch_bounds__(kCgBlock) void cg_apply_kernel(const T* __restrict__ r, const T* __restrict__ po,
                                                            T* __restrict__ pn, T* __restrict__ q, index_t pitch,
                                                            index_t core_off, index_t W, index_t H, unsigned gx,
                                                            index_t band_rows, T diag, T nc1, int vec_ok, int mirror,
                                                            S* sc, double* partials, unsigned* counter) {
  constexpr int N = CgVec<T>::N;
  using V = typename CgVec<T>::type;
  if (sc->status != kCgRunning) return;  // grid-uniform: nothing is stored, the ticket stays 0
  const T beta = T(sc->beta);
  const Strip<T> L(pitch, W, H, gx, band_rows, vec_ok);
  const T* rc = r + core_off;
  const T* oc = po + core_off;
  T* nc = pn + core_off;
  T* qc = q + core_off;
  const int nvalid = L.nvalid;

  // Row y of p_new = fma(beta, p_old, r): 0 outside the core, nothing loaded there.
  struct Row {
    V r, p;
  };
  auto ldrow = [&](index_t y) -> Row { return Row{L.ld(rc, y, nvalid), L.ld(oc, y, nvalid)}; };
  auto mk = [&](const Row& a) -> V {
    V o;
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = i < nvalid ? fma_t<T>(beta, a.p[i], a.r[i]) : T(0);
    return o;
  };
  // The (r, p_old) pairs of the columns just outside the strip on a core row.
  struct EdgeIn {
    T rl, pl, rr, pr;
    bool hl, hr;
  };
  auto lde = [&](index_t y) -> EdgeIn {
    EdgeIn e{T(0), T(0), T(0), T(0), false, false};
    const index_t o = y * pitch + L.x;
    if (L.left_load && L.x > 0) {
      e.rl = rc[o - 1];
      e.pl = oc[o - 1];
      e.hl = true;
    }
    if (L.right_load && L.x + N < W) {
      e.rr = rc[o + N];
      e.pr = oc[o + N];
      e.hr = true;
    }
    return e;
  };
  auto mke = [&](const EdgeIn& e) -> Edge<T> {
    return Edge<T>{e.hl ? fma_t<T>(beta, e.pl, e.rl) : T(0), e.hr ? fma_t<T>(beta, e.pr, e.rr) : T(0)};
  };
  const Row zero{V(T(0)), V(T(0))};
  const EdgeIn ezero{T(0), T(0), T(0), T(0), false, false};

  double acc = 0.0;
  if (L.any) {
    V up = L.y0 > 0 ? mk(ldrow(L.y0 - 1)) : V(T(0));
    V mid = mk(ldrow(L.y0));
    Edge<T> emid = mke(lde(L.y0));
#pragma unroll 1
    for (index_t y = L.y0; y < L.y1; y += kCh) {
      Row rn[kCh];
      EdgeIn en[kCh];
#pragma unroll
      for (int k = 0; k < kCh; ++k) {  // rows y + 1 .. y + kCh, inside the core only
        const index_t yn = y + k + 1;
        rn[k] = zero;
        en[k] = ezero;
        if (yn <= L.y1 && yn < H) rn[k] = ldrow(yn);
        if (yn < L.y1) en[k] = lde(yn);
      }
#pragma unroll
      for (int k = 0; k < kCh; ++k) {
        const V dn = mk(rn[k]);
        if (y + k < L.y1) {
          T left = lane_shift<kDppWaveShr1>(mid[N - 1]);
          T right = lane_shift<kDppWaveShl1>(mid[0]);
          left = L.lane == 0 ? emid.l : left;
          right = L.right_load ? emid.r : right;
          V out;
#pragma unroll
          for (int i = 0; i < N; ++i) {
            const T w = i == 0 ? left : mid[i > 0 ? i - 1 : 0];
            const T ea = i == N - 1 ? right : mid[i < N - 1 ? i + 1 : 0];
            T res;
            if constexpr (NEU) {  // only the global edges mirror, never a band or strip boundary
              const T c = mid[i];
              const T nn = (mirror & kMirrorTop) && y + k == 0 ? c : up[i];
              const T ss = (mirror & kMirrorBottom) && y + k == H - 1 ? c : dn[i];
              const T ww = (mirror & kMirrorLeft) && L.x + i == 0 ? c : w;
              const T ee = (mirror & kMirrorRight) && L.x + i == W - 1 ? c : ea;
              res = fma_t<T>(nc1, (nn + ss) + (ww + ee), diag * c);
            } else {
              res = fma_t<T>(nc1, (up[i] + dn[i]) + (w + ea), diag * mid[i]);
            }
            res = i < nvalid ? res : T(0);
            out[i] = res;
            acc = __builtin_fma(double(mid[i]), double(res), acc);
          }
          L.st(nc, y + k, mid);
          L.st(qc, y + k, out);
        }
        up = mid;
        mid = dn;
        emid = mke(en[k]);
      }
    }
  }

  const Total t = grid_reduce(acc, 0ull, partials, counter);
  if (!t.last || threadIdx.x != 0) return;
  const double pq = t.sum;
  sc->pq = pq;
  if (pq > 0.0 && pq <= 1.7976931348623157e308) {
    if constexpr (std::is_same<S, PcgScalars>::value) sc->alpha = sc->rz / pq;
    else sc->alpha = sc->rr / pq;
  } else {
    sc->alpha = 0.0;
    sc->status = kCgBreakdown;
  }
}

// ----------------------------------------------------------------- cg_update
// S: CgScalars (beta = rr' / rr) or PcgScalars (beta belongs to the preconditioner's dot epilogue).
template <typename T, typename S>
__global__ __launch_bounds__(kCgBlock) void cg_update_kernel(T* u, T* r, const T* __restrict__ p,
                                                             const T* __restrict__ q, index_t pitch, index_t core_off,
                                                             index_t W, index_t H, unsigned gx, index_t band_rows,
                                                             int vec_ok, S* sc, double* partials,
                                                             unsigned* counter) {
  constexpr int N = CgVec<T>::N;
  using V = typename CgVec<T>::type;
  using U = decltype(abs_bits(T(0)));
  if (sc->status != kCgRunning) return;  // grid-uniform
  const T alpha = T(sc->alpha);
  const T nalpha = -alpha;
  const Strip<T> L(pitch, W, H, gx, band_rows, vec_ok);
  T* uc = u + core_off;
  T* rc = r + core_off;
  const T* pc = p + core_off;
  const T* qc = q + core_off;
  const int nvalid = L.nvalid;

  U m = 0;
  double acc = 0.0;
  if (L.any) {
#pragma unroll 1
    for (index_t y = L.y0; y < L.y1; y += kCh) {
      V uv[kCh], rv[kCh], pv[kCh], qv[kCh];
#pragma unroll
      for (int k = 0; k < kCh; ++k) {
        uv[k] = rv[k] = pv[k] = qv[k] = V(T(0));
        if (y + k < L.y1) {
          uv[k] = L.ld(uc, y + k, nvalid);
          rv[k] = L.ld(rc, y + k, nvalid);
          pv[k] = L.ld(pc, y + k, nvalid);
          qv[k] = L.ld(qc, y + k, nvalid);
        }
      }
#pragma unroll
      for (int k = 0; k < kCh; ++k) {
        if (y + k < L.y1) {
          V un, rn;
#pragma unroll
          for (int i = 0; i < N; ++i) {
            un[i] = fma_t<T>(alpha, pv[k][i], uv[k][i]);
            T res = fma_t<T>(nalpha, qv[k][i], rv[k][i]);
            res = i < nvalid ? res : T(0);
            rn[i] = res;
            m = umax<U>(m, abs_bits(res));
            acc = __builtin_fma(double(res), double(res), acc);
          }
          L.st(uc, y + k, un);
          L.st(rc, y + k, rn);
        }
      }
    }
  }

  const Total t = grid_reduce(acc, static_cast<unsigned long long>(__double_as_longlong(from_bits(m))), partials, counter);
  if (!t.last || threadIdx.x != 0) return;
  const int it = sc->iteration + 1;
  if constexpr (std::is_same<S, CgScalars>::value) sc->beta = t.sum / sc->rr;
  sc->rr = t.sum;
  sc->linf = t.linf;
  sc->iteration = it;
  if (cg_within(sc->norm, t.sum, t.linf, sc->tol)) sc->status = kCgConverged;
  else if (it >= sc->max_iters) sc->status = kCgMaxIters;
}

struct CgGrid {
  unsigned gx = 1;
  index_t bands = 1, band_rows = kCh;
};

// Column groups over the width, then enough row bands for kCgWgsPerCu
// workgroups per CU; a band is a whole number of kCh-row chunks.
CgGrid cg_grid(const TileGeom& g, int elem_bytes) {
  CgGrid r;
  const index_t group_cols = index_t(kCgWaves) * kWaveSize * (16 / elem_bytes);
  r.gx = unsigned(std::max<index_t>(1, (g.width + group_cols - 1) / group_cols));
  const index_t target = index_t(kCgWgsPerCu) * std::max(1, device_cu_count());
  const index_t chunks = std::max<index_t>(1, (g.height + kCh - 1) / kCh);
  const index_t want = std::max<index_t>(1, std::min<index_t>(chunks, target / r.gx));
  r.band_rows = (chunks + want - 1) / want * kCh;
  r.bands = std::max<index_t>(1, (g.height + r.band_rows - 1) / r.band_rows);
  return r;
}

template <typename T>
bool aligned16(const T* tile, const TileGeom& g) {
  return reinterpret_cast<std::uintptr_t>(tile + g.core_offset()) % 16 == 0;
}

// The sides of a CG launch are the solve's: ring or mirror.
int mirror_mask(const char* who, const GhostSides& sd) {
  for (int code : {sd.top, sd.bottom, sd.left, sd.right})
    MXS_CHECK(code == kGhostRing || code == kGhostMirror, who << ": a side is ring (0) or mirror (+1), got " << code);
  return (sd.top ? kMirrorTop : 0) | (sd.bottom ? kMirrorBottom : 0) | (sd.left ? kMirrorLeft : 0) |
         (sd.right ? kMirrorRight : 0);
}

// The checks every launcher shares; returns the grid.
template <typename T>
CgGrid check(const char* who, const TileGeom& g, std::initializer_list<const T*> tiles, const void* scalars,
             const double* partials, const unsigned* counter) {
  MXS_CHECK(g.halo_x >= 1 && g.halo_y >= 1, who << ": the tile has no ghost ring (it needs one at least 1 deep)");
  MXS_CHECK(g.width >= 1 && g.height >= 1 && g.pitch >= g.x_origin + g.total_width(), who << ": bad tile geometry");
  for (const T* t : tiles)
    MXS_CHECK(t != nullptr && reinterpret_cast<std::uintptr_t>(t) % sizeof(T) == 0,
              who << ": needs every tile, element-aligned");
  MXS_CHECK(scalars && partials && counter && reinterpret_cast<std::uintptr_t>(scalars) % sizeof(double) == 0 &&
                reinterpret_cast<std::uintptr_t>(partials) % sizeof(double) == 0 &&
                reinterpret_cast<std::uintptr_t>(counter) % sizeof(unsigned) == 0,
            who << ": needs the scalar block, the partials and the ticket, aligned");
  const CgGrid cg = cg_grid(g, int(sizeof(T)));
  const index_t grid = index_t(cg.gx) * cg.bands;
  MXS_CHECK(grid <= index_t(cg_grid_size(g)) && grid < (index_t(1) << 31), who << ": grid size");
  return cg;
}

// The three launchers, once over the scalar block S (CgScalars: cg_*,
// PcgScalars: pcg_*). `who` is the public function's name, a literal: it
// prefixes the check messages and is what last_cg_dispatch() reports.
// p: the first direction's tile, nullptr with PcgScalars (none is stored).
template <typename T, typename S>
void launch_start(const char* who, const T* u, const T* g, T* r, T* p, const TileGeom& geom, Stencil5Coeffs c,
                  S* scalars, double* partials, unsigned* counter, hipStream_t s, GhostSides sides) {
  constexpr bool kPcg = std::is_same<S, PcgScalars>::value;
  const CgGrid cg = kPcg ? check<T>(who, geom, {u, g, r}, scalars, partials, counter)
                         : check<T>(who, geom, {u, g, r, p}, scalars, partials, counter);
  if (kPcg) MXS_CHECK(p == nullptr && u != r && g != r && u != g, who << ": u, g and r must be three tiles");
  else MXS_CHECK(u != r && u != p && g != r && g != p && r != p, who << ": u, g, r and p must be four tiles (r != p)");
  constexpr int N = CgVec<T>::N;
  const int vec_ok = geom.pitch % N == 0 && aligned16(u, geom) && aligned16(g, geom) && aligned16(r, geom) &&
                     (kPcg || aligned16(p, geom));
  const int mirror = mirror_mask(who, sides);
  auto* kernel = mirror ? cg_start_kernel<T, S, true> : cg_start_kernel<T, S, false>;
  kernel<<<unsigned(index_t(cg.gx) * cg.bands), kCgBlock, 0, s>>>(u, g, r, p, geom.pitch, geom.core_offset(), geom.width,
                                                                  geom.height, cg.gx, cg.band_rows, T(c.center),
                                                                  T(c.neighbor), vec_ok, mirror, scalars, partials,
                                                                  counter);
  g_last_cg = who;
  MXS_HIP_CHECK_LAUNCH();
}

// The start of an implicit heat step: launch_start with g an output and the
// optional source tile q (nullptr: the no-source kernel, q is never read).
template <typename T, typename S>
void launch_heat_start(const char* who, const T* u, const T* q, T* g, T* r, T* p, const TileGeom& geom,
                       const HeatCoeffs& hc, S* scalars, double* partials, unsigned* counter, hipStream_t s,
                       GhostSides sides) {
  constexpr bool kPcg = std::is_same<S, PcgScalars>::value;
  const CgGrid cg = kPcg ? check<T>(who, geom, {u, g, r}, scalars, partials, counter)
                         : check<T>(who, geom, {u, g, r, p}, scalars, partials, counter);
  MXS_CHECK(q == nullptr || reinterpret_cast<std::uintptr_t>(q) % sizeof(T) == 0, who << ": q must be element-aligned");
  if (kPcg) MXS_CHECK(p == nullptr && u != r && g != r && u != g, who << ": u, g and r must be three tiles");
  else MXS_CHECK(u != r && u != p && g != r && g != p && r != p && u != g, who << ": u, g, r and p must be four tiles (r != p)");
  MXS_CHECK(q == nullptr || (q != g && q != r && q != p), who << ": the source q must not be one of the written tiles g, r, p");
  constexpr int N = CgVec<T>::N;
  const int vec_ok = geom.pitch % N == 0 && aligned16(u, geom) && aligned16(g, geom) && aligned16(r, geom) &&
                     (kPcg || aligned16(p, geom)) && (q == nullptr || aligned16(q, geom));
  const int mirror = mirror_mask(who, sides);
  auto* kernel = q ? (mirror ? cg_heat_start_kernel<T, S, true, true> : cg_heat_start_kernel<T, S, false, true>)
                   : (mirror ? cg_heat_start_kernel<T, S, true, false> : cg_heat_start_kernel<T, S, false, false>);
  kernel<<<unsigned(index_t(cg.gx) * cg.bands), kCgBlock, 0, s>>>(u, q, g, r, p, geom.pitch, geom.core_offset(),
                                                                  geom.width, geom.height, cg.gx, cg.band_rows, T(hc.c1),
                                                                  T(hc.a), T(hc.b), T(hc.s), vec_ok, mirror, scalars,
                                                                  partials, counter);
  g_last_cg = who;
  MXS_HIP_CHECK_LAUNCH();
}

// r: the residual, or with PcgScalars z = M r.
template <typename T, typename S>
void launch_apply(const char* who, const T* r, const T* p_old, T* p_new, T* q, const TileGeom& geom, Stencil5Coeffs c,
                  S* scalars, double* partials, unsigned* counter, hipStream_t s, GhostSides sides) {
  const CgGrid cg = check<T>(who, geom, {r, p_old, p_new, q}, scalars, partials, counter);
  MXS_CHECK(p_old != p_new, who << ": p_old != p_new (neighbouring workgroups still read p_old: pass the other "
                                   "buffer of the ping-pong pair)");
  MXS_CHECK(r != p_new && r != q && p_old != q && p_new != q,
            who << ": " << (std::is_same<S, PcgScalars>::value ? "z" : "r") << ", p_old, p_new and q must be four tiles");
  constexpr int N = CgVec<T>::N;
  const int vec_ok = geom.pitch % N == 0 && aligned16(r, geom) && aligned16(p_old, geom) && aligned16(p_new, geom) &&
                     aligned16(q, geom);
  const int mirror = mirror_mask(who, sides);
  auto* kernel = mirror ? cg_apply_kernel<T, S, true> : cg_apply_kernel<T, S, false>;
  kernel<<<unsigned(index_t(cg.gx) * cg.bands), kCgBlock, 0, s>>>(r, p_old, p_new, q, geom.pitch, geom.core_offset(),
                                                                  geom.width, geom.height, cg.gx, cg.band_rows,
                                                                  T(1.0 - c.center), T(-c.neighbor), vec_ok, mirror,
                                                                  scalars, partials, counter);
  g_last_cg = who;
  MXS_HIP_CHECK_LAUNCH();
}

template <typename T, typename S>
void launch_update(const char* who, T* u, T* r, const T* p, const T* q, const TileGeom& geom, S* scalars,
                   double* partials, unsigned* counter, hipStream_t s) {
  const CgGrid cg = check<T>(who, geom, {u, r, p, q}, scalars, partials, counter);
  MXS_CHECK(u != r && u != p && u != q && r != p && r != q && p != q, who << ": u, r, p and q must be four tiles");
  constexpr int N = CgVec<T>::N;
  const int vec_ok = geom.pitch % N == 0 && aligned16(u, geom) && aligned16(r, geom) && aligned16(p, geom) &&
                     aligned16(q, geom);
  cg_update_kernel<T, S><<<unsigned(index_t(cg.gx) * cg.bands), kCgBlock, 0, s>>>(
      u, r, p, q, geom.pitch, geom.core_offset(), geom.width, geom.height, cg.gx, cg.band_rows, vec_ok, scalars,
      partials, counter);
  g_last_cg = who;
  MXS_HIP_CHECK_LAUNCH();
}

}  // namespace

const char* last_cg_dispatch() { return g_last_cg.load(); }

int cg_grid_size(const TileGeom& g) {
  const CgGrid a = cg_grid(g, 4), b = cg_grid(g, 8);
  return int(std::max<index_t>(a.gx * a.bands, b.gx * b.bands));
}

template <typename T>
void cg_start(const T* u, const T* g, T* r, T* p, const TileGeom& geom, Stencil5Coeffs c, CgScalars* scalars,
              double* partials, unsigned* counter, hipStream_t s, GhostSides sides) {
  launch_start<T>("cg_start", u, g, r, p, geom, c, scalars, partials, counter, s, sides);
}

template <typename T>
void cg_apply(const T* r, const T* p_old, T* p_new, T* q, const TileGeom& geom, Stencil5Coeffs c, CgScalars* scalars,
              double* partials, unsigned* counter, hipStream_t s, GhostSides sides) {
  launch_apply<T>("cg_apply", r, p_old, p_new, q, geom, c, scalars, partials, counter, s, sides);
}

template <typename T>
void cg_update(T* u, T* r, const T* p, const T* q, const TileGeom& geom, CgScalars* scalars, double* partials,
               unsigned* counter, hipStream_t s) {
  launch_update<T>("cg_update", u, r, p, q, geom, scalars, partials, counter, s);
}

// -------------------------------------------------------- preconditioned CG
template <typename T>
void pcg_start(const T* u, const T* g, T* r, const TileGeom& geom, Stencil5Coeffs c, PcgScalars* scalars,
               double* partials, unsigned* counter, hipStream_t s, GhostSides sides) {
  launch_start<T>("pcg_start", u, g, r, static_cast<T*>(nullptr), geom, c, scalars, partials, counter, s, sides);
}

template <typename T>
void pcg_apply(const T* z, const T* p_old, T* p_new, T* q, const TileGeom& geom, Stencil5Coeffs c, PcgScalars* scalars,
               double* partials, unsigned* counter, hipStream_t s, GhostSides sides) {
  launch_apply<T>("pcg_apply", z, p_old, p_new, q, geom, c, scalars, partials, counter, s, sides);
}

template <typename T>
void pcg_update(T* u, T* r, const T* p, const T* q, const TileGeom& geom, PcgScalars* scalars, double* partials,
                unsigned* counter, hipStream_t s) {
  launch_update<T>("pcg_update", u, r, p, q, geom, scalars, partials, counter, s);
}

// ------------------------------------------------------ implicit heat steps
template <typename T>
void cg_heat_start(const T* u, const T* q, T* g, T* r, T* p, const TileGeom& geom, const HeatCoeffs& hc,
                   CgScalars* scalars, double* partials, unsigned* counter, hipStream_t s, GhostSides sides) {
  launch_heat_start<T>("cg_heat_start", u, q, g, r, p, geom, hc, scalars, partials, counter, s, sides);
}

template <typename T>
void pcg_heat_start(const T* u, const T* q, T* g, T* r, const TileGeom& geom, const HeatCoeffs& hc,
                    PcgScalars* scalars, double* partials, unsigned* counter, hipStream_t s, GhostSides sides) {
  launch_heat_start<T>("pcg_heat_start", u, q, g, r, static_cast<T*>(nullptr), geom, hc, scalars, partials, counter, s,
                       sides);
}

#define MXS_HEAT_INSTANTIATE(T)                                                                                       \
  template void cg_heat_start<T>(const T*, const T*, T*, T*, T*, const TileGeom&, const HeatCoeffs&, CgScalars*,      \
                                 double*, unsigned*, hipStream_t, GhostSides);                                        \
  template void pcg_heat_start<T>(const T*, const T*, T*, T*, const TileGeom&, const HeatCoeffs&, PcgScalars*,        \
                                  double*, unsigned*, hipStream_t, GhostSides);
MXS_HEAT_INSTANTIATE(float)
MXS_HEAT_INSTANTIATE(double)
#undef MXS_HEAT_INSTANTIATE

#define MXS_CG_INSTANTIATE(T)                                                                                    \
  template void cg_start<T>(const T*, const T*, T*, T*, const TileGeom&, Stencil5Coeffs, CgScalars*, double*,       \
                            unsigned*, hipStream_t, GhostSides);                                                    \
  template void cg_apply<T>(const T*, const T*, T*, T*, const TileGeom&, Stencil5Coeffs, CgScalars*, double*,       \
                            unsigned*, hipStream_t, GhostSides);                                                    \
  template void cg_update<T>(T*, T*, const T*, const T*, const TileGeom&, CgScalars*, double*, unsigned*, hipStream_t); \
  template void pcg_start<T>(const T*, const T*, T*, const TileGeom&, Stencil5Coeffs, PcgScalars*, double*, unsigned*, \
                             hipStream_t, GhostSides);                                                                 \
  template void pcg_apply<T>(const T*, const T*, T*, T*, const TileGeom&, Stencil5Coeffs, PcgScalars*, double*,       \
                             unsigned*, hipStream_t, GhostSides);                                                      \
  template void pcg_update<T>(T*, T*, const T*, const T*, const TileGeom&, PcgScalars*, double*, unsigned*, hipStream_t);
MXS_CG_INSTANTIATE(float)
MXS_CG_INSTANTIATE(double)
#undef MXS_CG_INSTANTIATE

}  // namespace kernels
}  // namespace mxs
